// Head conv (3x3, 3->F) and fused tail (3x3, F->3r^2) + skip (5x5, 3->3r^2) + PixelShuffle(r) + mean,
// forward and backward (gfx950).  Reference ops replaced: BASIC_MODEL.forward, models/basic_wdsr_b.py:85-93
// (x - mean; head :32-42; tail :55-64; skip :66-78; shuf :80-83; + mean :92) and their autograd backward.
//
// The LR image is NCHW fp32 in HBM (the reference's layout) and is staged in LDS as [pixel][4]:
// 3 colours minus the mean (zero outside the image = the conv's zero padding of x - mean) plus a ones
// channel that carries the bias.  One 8-element fragment chunk = two horizontally adjacent pixels.
// The HR output is written straight from the accumulator: with out^T tiles (rows = conv channel
// c*r*r + i*r + j, lanes = LR pixel) the 4 registers of a group are the r = 4 sub-columns j of one HR row,
// so PixelShuffle is pure addressing (no intermediate buffer, no cross-lane traffic).
#pragma once
#include "wdsr_block.h"

template <int F_, int R_>
struct EndsCfg {
  static constexpr int F = F_, R = R_;
  static constexpr int CO = 3 * R * R, NT = (CO + 31) / 32, COP = (CO + 7) / 8 * 8, CC = COP / 8, FC = F / 8;
  static constexpr int KST = (9 * FC + 15 + 1) / 2, KSTB = (9 * CC + 1) / 2;
  static constexpr int TH = 12, TW = 24, HW = TW + 2, HH = TH + 2, NPXH = HW * HH, NPXH_PAD = (NPXH + 31) / 32 * 32;
  static constexpr int NPT_O = (TH / 4) * (TW / 8), NPXC = TH * TW;
  static constexpr int FT_ELEMS = (NPXH_PAD + 2) * F;           // feature (or dy) tile with 1-px halo
  static constexpr int DC_ELEMS = (NPXH_PAD + 2) * COP;         // dconv tile with 1-px halo
  static constexpr int DCC_ELEMS = (NPXC + 2) * COP;            // dconv core tile
  static constexpr int DYC_ELEMS = (NPXC + 2) * F;              // dy core tile (head wgrad)
  template <int P> struct Img {                                 // LR image tile with P-px halo
    static constexpr int IW = TW + 2 * P, IH = TH + 2 * P, NPI = IW * IH, ELEMS = (NPI + 8) * 4;
  };
  static constexpr int TAIL_TILES = 14 * NT;                    // 9 taps + 5 skip rows, NT row tiles each
};

// 8 elements from an LDS image at an offset that is only 4-element aligned
template <typename T> SR_DEV typename FragOf<T>::type lds_chunk_half(const T* img, int off) {
  typedef typename FragOf<T>::half_type HalfT;
  const HalfT lo = *reinterpret_cast<const HalfT*>(img + off);
  const HalfT hi = *reinterpret_cast<const HalfT*>(img + off + 4);
  typename FragOf<T>::type f;
  f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3];
  f[4] = hi[0]; f[5] = hi[1]; f[6] = hi[2]; f[7] = hi[3];
  return f;
}

// Staging helpers.  Every helper issues the global loads of up to SR_STAGE_BATCH iterations before the first
// LDS store of the batch, so a tile costs a couple of HBM round trips instead of one per iteration.
#define SR_STAGE_BATCH 4

template <typename T, typename E, int P, int NTHREADS = 256>
SR_DEV void stage_img(T* XI, const float* __restrict__ ximg, float mean, int H, int W, int ty0, int tx0, int tid) {
  typedef typename FragOf<T>::half_type HalfT;
  typedef typename E::template Img<P> I;
  const size_t plane = (size_t)H * W;
  constexpr int TOTAL = I::NPI + 8, ITER = (TOTAL + NTHREADS - 1) / NTHREADS;
#pragma unroll
  for (int b0 = 0; b0 < ITER; b0 += SR_STAGE_BATCH) {
    float v[SR_STAGE_BATCH][3];
#pragma unroll
    for (int b = 0; b < SR_STAGE_BATCH; ++b) {
      const int ip = tid + (b0 + b) * NTHREADS;
      v[b][0] = 0.f; v[b][1] = 0.f; v[b][2] = 0.f;
      if (b0 + b < ITER && ip < I::NPI) {
        const int iy = ip / I::IW, ix = ip - iy * I::IW;
        const int Y = ty0 - P + iy, X = tx0 - P + ix;
        if (Y >= 0 && Y < H && X >= 0 && X < W) {
          const size_t o = (size_t)Y * W + X;
          v[b][0] = ximg[o] - mean;
          v[b][1] = ximg[plane + o] - mean;
          v[b][2] = ximg[2 * plane + o] - mean;
        }
      }
    }
#pragma unroll
    for (int b = 0; b < SR_STAGE_BATCH; ++b) {
      const int ip = tid + (b0 + b) * NTHREADS;
      if (b0 + b < ITER && ip < TOTAL) {
        HalfT h;
        h[0] = (T)v[b][0]; h[1] = (T)v[b][1]; h[2] = (T)v[b][2]; h[3] = (T)1.f;
        *reinterpret_cast<HalfT*>(XI + ip * 4) = h;
      }
    }
  }
}

// rows p < NLIVE of a [NROWS][CH] LDS image = pixels (y0 + p / RW, x0 + p % RW) of an NHWC tensor, zero elsewhere
template <typename T, int CH, int RW, int NROWS, int NLIVE, int NTHREADS>
SR_DEV void stage_rows(T* dst, const T* __restrict__ src, int H, int W, int y0, int x0, int tid) {
  typedef typename FragOf<T>::type FragT;
  constexpr int NC = CH / 8, TOTAL = NROWS * NC, ITER = (TOTAL + NTHREADS - 1) / NTHREADS;
#pragma unroll
  for (int b0 = 0; b0 < ITER; b0 += SR_STAGE_BATCH) {
    FragT v[SR_STAGE_BATCH];
#pragma unroll
    for (int b = 0; b < SR_STAGE_BATCH; ++b) {
      const int idx = tid + (b0 + b) * NTHREADS;
      const int p = idx / NC, c = idx - p * NC;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[b][j] = (T)0.f;
      if (b0 + b < ITER && p < NLIVE) {
        const int py = p / RW, px = p - py * RW;
        const int Y = y0 + py, X = x0 + px;
        if (Y >= 0 && Y < H && X >= 0 && X < W) v[b] = *reinterpret_cast<const FragT*>(src + ((size_t)Y * W + X) * CH + c * 8);
      }
    }
#pragma unroll
    for (int b = 0; b < SR_STAGE_BATCH; ++b) {
      const int idx = tid + (b0 + b) * NTHREADS;
      if (b0 + b < ITER && idx < TOTAL) *reinterpret_cast<FragT*>(dst + idx * 8) = v[b];
    }
  }
}

// feature / gradient tile with a 1-pixel halo: [NPXH_PAD + 2][CH] (CH multiple of 8), zero outside
template <typename T, typename E, int CH, int NTHREADS = 256>
SR_DEV void stage_halo(T* dst, const T* __restrict__ src, int H, int W, int ty0, int tx0, int tid) {
  stage_rows<T, CH, E::HW, E::NPXH_PAD + 2, E::NPXH, NTHREADS>(dst, src, H, W, ty0 - 1, tx0 - 1, tid);
}

template <typename T, typename E, int CH, int NTHREADS = 256>
SR_DEV void stage_core(T* dst, const T* __restrict__ src, int H, int W, int ty0, int tx0, int tid) {
  stage_rows<T, CH, E::TW, E::NPXC + 2, E::NPXC, NTHREADS>(dst, src, H, W, ty0, tx0, tid);
}

// un-shuffle the HR gradient (NCHW fp32, N x 3 x RH x RW) into a dconv tile [px][COP]:
// channel c*R*R + i*R + j of LR pixel (Y, X) = dout[c][Y*R + i][X*R + j].  HALO = 1: tile with halo,
// HALO = 0: core tile.
// LOSS folds the trainers' loss into this read (pretrain.py:73-77 L1, train_video_superresolution.py:43-53
// Charbonnier): `dout` is then the network OUTPUT sr, `hr` the target, and the gradient is formed on the fly,
//   LOSS 1:  g = sign(sr - hr) * gscale           (torch's l1_loss backward; gscale = upstream / numel)
//   LOSS 2:  g = (sr - hr) / sqrt((sr - hr)^2 + 1e-12) * gscale
// while `lsum` collects this thread's share of sum |sr - hr| (resp. sum sqrt(d^2 + 1e-12)) over the CORE pixels
// (each HR pixel is a core pixel of exactly one tile): the 14 MB HR gradient never exists in HBM.
struct LossIn {
  const float* hr;
  float gscale;
};
template <int LOSS> SR_DEV float loss_grad(float q, float h, float gscale, float& term) {
  const float d = q - h;
  if constexpr (LOSS == 1) {
    term = fabsf(d);
    return d == 0.f ? 0.f : __builtin_copysignf(gscale, d);
  } else {
    const float s = sqrtf(d * d + 1e-12f);
    term = s;
    return d / s * gscale;
  }
}
template <typename T, typename E, int HALO, int NTHREADS = 256, int LOSS = 0>
SR_DEV void stage_dconv(T* DC, const float* __restrict__ dout, int H, int W, int ty0, int tx0, int tid, LossIn li = LossIn{nullptr, 0.f},
                        float* lsum = nullptr) {
  constexpr int R = E::R;
  constexpr int NPX = HALO ? (E::NPXH_PAD + 2) : (E::NPXC + 2);
  constexpr int NLIVE = HALO ? E::NPXH : E::NPXC;
  constexpr int TWW = HALO ? E::HW : E::TW;
  const unsigned hrw = (unsigned)W * R, plane = (unsigned)H * R * hrw;   // one image: 32-bit offsets from a uniform base
  constexpr int ROWS = 3 * R;                       // (colour, sub-row) pairs per pixel
  constexpr int BATCH = LOSS ? (R == 2 ? 1 : 2) : SR_STAGE_BATCH;   // loads in flight per thread (the loss fold reads two tensors)
  constexpr int TOTAL = NPX * ROWS, ITER = (TOTAL + NTHREADS - 1) / NTHREADS;
#pragma unroll
  for (int b0 = 0; b0 < ITER; b0 += BATCH) {
    float v[BATCH][R];
#pragma unroll
    for (int b = 0; b < BATCH; ++b) {
      const int idx = tid + (b0 + b) * NTHREADS;
      const int p = idx / ROWS, cr = idx - p * ROWS;
      const int c = cr / R, si = cr - c * R;
#pragma unroll
      for (int j = 0; j < R; ++j) v[b][j] = 0.f;
      if (b0 + b < ITER && p < NLIVE) {
        const int py = p / TWW, px = p - py * TWW;
        const int Y = ty0 - HALO + py, X = tx0 - HALO + px;
        if (Y >= 0 && Y < H && X >= 0 && X < W) {
          const unsigned off = c * plane + ((unsigned)Y * R + si) * hrw + (unsigned)X * R;
          const float* s = dout + off;
          if constexpr (R == 4) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(s);
            v[b][0] = q[0]; v[b][1] = q[1]; v[b][2] = q[2]; v[b][3] = q[3];
          } else {
#pragma unroll
            for (int j = 0; j < R; ++j) v[b][j] = s[j];
          }
          if constexpr (LOSS != 0) {
            float h[R];
            if constexpr (R == 4) {
              const f32x4 q = *reinterpret_cast<const f32x4*>(li.hr + off);
              h[0] = q[0]; h[1] = q[1]; h[2] = q[2]; h[3] = q[3];
            } else {
#pragma unroll
              for (int j = 0; j < R; ++j) h[j] = li.hr[off + j];
            }
            const bool core = !HALO || (py >= 1 && py <= E::TH && px >= 1 && px <= E::TW);
#pragma unroll
            for (int j = 0; j < R; ++j) {
              float term;
              v[b][j] = loss_grad<LOSS>(v[b][j], h[j], li.gscale, term);
              if (core && lsum) *lsum += term;
            }
          }
        }
      }
    }
#pragma unroll
    for (int b = 0; b < BATCH; ++b) {
      const int idx = tid + (b0 + b) * NTHREADS;
      if (b0 + b < ITER && idx < TOTAL) {
        const int p = idx / ROWS, cr = idx - p * ROWS;
        const int c = cr / R, si = cr - c * R;
        T* d = DC + p * E::COP + c * R * R + si * R;
        if constexpr (R == 4) {
          typename FragOf<T>::half_type hv;
          hv[0] = (T)v[b][0]; hv[1] = (T)v[b][1]; hv[2] = (T)v[b][2]; hv[3] = (T)v[b][3];
          *reinterpret_cast<typename FragOf<T>::half_type*>(d) = hv;
        } else {
#pragma unroll
          for (int j = 0; j < R; ++j) d[j] = (T)v[b][j];
        }
      }
    }
  }
  if constexpr (E::COP > E::CO) {                    // zero the padding channels
    for (int idx = tid; idx < NPX * (E::COP - E::CO); idx += NTHREADS) {
      const int p = idx / (E::COP - E::CO), k = idx - p * (E::COP - E::CO);
      DC[p * E::COP + E::CO + k] = (T)0.f;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// head forward: y[n, Y, X, :] = conv3x3(x - mean) + b   (NCHW fp32 image -> NHWC T features)
// ---------------------------------------------------------------------------------------------
template <typename T, int F>
__global__ __launch_bounds__(256) void sr_head_fwd_kernel(const float* __restrict__ ximg, T* __restrict__ y,
                                                          const T* __restrict__ wblob, float mean, int H, int W,
                                                          int tiles_x) {
  typedef EndsCfg<F, 4> E;
  typedef typename E::template Img<1> I;
  typedef typename FragOf<T>::half_type HalfT;
  __shared__ __attribute__((aligned(16))) T XI[I::ELEMS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int n = blockIdx.y, tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * E::TH, tx0 = (tile % tiles_x) * E::TW;
  stage_img<T, E, 1>(XI, ximg + (size_t)n * 3 * H * W, mean, H, W, ty0, tx0, tid);
  __syncthreads();
  for (int ot = wave; ot < E::NPT_O; ot += 4) {
    const int oy = (ot / (E::TW / 8)) * 4 + (r >> 3), ox = (ot % (E::TW / 8)) * 8 + (r & 7);
    f32x16 acc = zero16();
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int q = 2 * s + hh, ky = q >> 1, m = q & 1;
      acc = mma16<T>(load_wfrag<T>(wblob, s, lane), lds_chunk_half<T>(XI, ((oy + ky) * I::IW + ox + 2 * m) * 4), acc);
    }
    const int Y = ty0 + oy, X = tx0 + ox;
    if (Y < H && X < W) {
      T* yo = y + (((size_t)n * H + Y) * W + X) * F;
#pragma unroll
      for (int g = 0; g < E::FC; ++g) stream_store(reinterpret_cast<HalfT*>(yo + g * 8 + hh * 4), acc_group<T>(acc, g));
    }
  }
}

// ---------------------------------------------------------------------------------------------
// tail forward: out = PixelShuffle_R( conv3x3(feat; Wt) + conv5x5(x - mean; Ws) + bt + bs ) + mean
// (the three constants ride on the image's ones channel at the skip's centre tap)
// ---------------------------------------------------------------------------------------------
// eight waves (round 3): the tile's nine pixel tiles are two rounds instead of three, two waves per SIMD (four waves before: one per SIMD)
constexpr int SR_TAIL_FWD_THREADS = 512;
template <typename T, int F, int R>
__global__ __launch_bounds__(SR_TAIL_FWD_THREADS) void sr_tail_fwd_kernel(const T* __restrict__ feat, const float* __restrict__ ximg,
                                                          float* __restrict__ out, const T* __restrict__ wblob,
                                                          float mean, int H, int W, int tiles_x) {
  typedef EndsCfg<F, R> E;
  typedef typename E::template Img<2> I;
  typedef typename FragOf<T>::type FragT;
  __shared__ __attribute__((aligned(16))) T smem[E::FT_ELEMS + I::ELEMS];
  T* const FT = smem;
  constexpr int XI0 = E::FT_ELEMS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int n = blockIdx.y, tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * E::TH, tx0 = (tile % tiles_x) * E::TW;
  stage_halo<T, E, F, SR_TAIL_FWD_THREADS>(FT, feat + (size_t)n * H * W * F, H, W, ty0, tx0, tid);
  stage_img<T, E, 2, SR_TAIL_FWD_THREADS>(smem + XI0, ximg + (size_t)n * 3 * H * W, mean, H, W, ty0, tx0, tid);
  __syncthreads();
  constexpr bool HOIST = (sizeof(T) == 2) && (E::NT * E::KST <= 42);
  const T* const wblob0 = wblob;
  for (int ot = wave; ot < E::NPT_O; ot += SR_TAIL_FWD_THREADS / 64) {
    wblob = weights_for_tile<HOIST>(wblob0);
    const int oy = (ot / (E::TW / 8)) * 4 + (r >> 3), ox = (ot % (E::TW / 8)) * 8 + (r & 7);
    const int hbase = oy * E::HW + ox;
    f32x16 acc[E::NT];
#pragma unroll
    for (int ti = 0; ti < E::NT; ++ti) acc[ti] = zero16();
#pragma unroll
    for (int s = 0; s < E::KST; ++s) {
      const int q = 2 * s + hh;
      FragT b;
      if (2 * s + 1 < 9 * E::FC) {                          // both lane halves read feature chunks
        const int tap = q / E::FC, c = q - tap * E::FC;
        b = lds_chunk<T>(smem, (hbase + (tap / 3) * E::HW + (tap % 3)) * F + c * 8);
      } else {
        int off;
        if (q < 9 * E::FC) {
          const int tap = q / E::FC, c = q - tap * E::FC;
          off = (hbase + (tap / 3) * E::HW + (tap % 3)) * F + c * 8;
        } else {
          int qs = q - 9 * E::FC;
          if (qs >= 15) qs = 0;                             // zero weights there
          const int ky = qs / 3, m = qs - ky * 3;
          off = XI0 + ((oy + ky) * I::IW + ox + 2 * m) * 4;
        }
        b = lds_chunk_half<T>(smem, off);
      }
#pragma unroll
      for (int ti = 0; ti < E::NT; ++ti) acc[ti] = mma16<T>(load_wfrag<T>(wblob, ti * E::KST + s, lane), b, acc[ti]);
    }
    const int Y = ty0 + oy, X = tx0 + ox;
    if (Y < H && X < W) {
      const size_t hrw = (size_t)W * R, plane = (size_t)H * R * hrw;
      float* o = out + (size_t)n * 3 * plane;
#pragma unroll
      for (int ti = 0; ti < E::NT; ++ti) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int ch0 = 32 * ti + 8 * g + 4 * hh;         // rows ch0 .. ch0+3 live in regs 4g..4g+3
          if constexpr (R == 4) {
            if (ch0 < E::CO) {
              const int c = ch0 >> 4, si = (ch0 >> 2) & 3;
              f32x4 v;
              v[0] = acc[ti][4 * g]; v[1] = acc[ti][4 * g + 1]; v[2] = acc[ti][4 * g + 2]; v[3] = acc[ti][4 * g + 3];
              *reinterpret_cast<f32x4*>(o + c * plane + ((size_t)Y * 4 + si) * hrw + (size_t)X * 4) = v;
            }
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int ch = ch0 + j;
              if (ch < E::CO) {
                const int c = ch / (R * R), rem = ch - c * R * R, si = rem / R, sj = rem - si * R;
                o[c * plane + ((size_t)Y * R + si) * hrw + (size_t)X * R + sj] = acc[ti][4 * g + j];
              }
            }
          }
        }
      }
    }
  }
}

// sum `v` over the workgroup (plain LDS stores, `red` = NTHREADS / 64 floats) and let thread 0 write it
template <int NTHREADS> SR_DEV void wg_sum_store(float v, float* red, float* out, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int i = 0; i < NTHREADS / 64; ++i) t += red[i];
    *out = t;
  }
}

// ---------------------------------------------------------------------------------------------
// tail backward-data: dfeat[px, f] = sum_{u, ch} Wt[ch, f, 8-u] dconv[px + u - 1, ch]
// ---------------------------------------------------------------------------------------------
template <typename T, int F, int R, int LOSS = 0>
__global__ __launch_bounds__(256) void sr_tail_bwd_data_kernel(const float* __restrict__ dout, T* __restrict__ dfeat,
                                                               const T* __restrict__ wblob, int H, int W,
                                                               int tiles_x, LossIn li) {
  typedef EndsCfg<F, R> E;
  typedef typename FragOf<T>::half_type HalfT;
  __shared__ __attribute__((aligned(16))) T DC[E::DC_ELEMS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int n = blockIdx.y, tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * E::TH, tx0 = (tile % tiles_x) * E::TW;
  li.hr += LOSS ? (size_t)n * 3 * H * R * W * R : 0;
  stage_dconv<T, E, 1, 256, LOSS>(DC, dout + (size_t)n * 3 * H * R * W * R, H, W, ty0, tx0, tid, li, nullptr);
  __syncthreads();
  const T* wt = wblob + (size_t)E::NT * E::KST * 512;        // backward-data section follows the forward one
  constexpr bool HOIST = (sizeof(T) == 2);
  const T* const wt0 = wt;
  for (int ot = wave; ot < E::NPT_O; ot += 4) {
    wt = weights_for_tile<HOIST>(wt0);
    const int oy = (ot / (E::TW / 8)) * 4 + (r >> 3), ox = (ot % (E::TW / 8)) * 8 + (r & 7);
    const int hbase = oy * E::HW + ox;
    f32x16 acc = zero16();
#pragma unroll
    for (int s = 0; s < E::KSTB; ++s) {
      const int q = 2 * s + hh;
      int off = hbase * E::COP;
      if (q < 9 * E::CC) {
        const int u = q / E::CC, c = q - u * E::CC;
        off = (hbase + (u / 3) * E::HW + (u % 3)) * E::COP + c * 8;
      }
      acc = mma16<T>(load_wfrag<T>(wt, s, lane), lds_chunk<T>(DC, off), acc);
    }
    const int Y = ty0 + oy, X = tx0 + ox;
    if (Y < H && X < W) {
      T* o = dfeat + (((size_t)n * H + Y) * W + X) * F;
#pragma unroll
      for (int g = 0; g < E::FC; ++g) stream_store(reinterpret_cast<HalfT*>(o + g * 8 + hh * 4), acc_group<T>(acc, g));
    }
  }
}

// ---------------------------------------------------------------------------------------------
// tail weight gradients.  14 waves: wave g < 9 owns tap g of the 3x3 tail conv, wave 9 + ky owns skip row ky;
// each keeps its NT accumulator tiles [conv channel rows, input columns] in registers over every pixel
// tile the workgroup walks (no cross-wave reduction), pixels contracted through transposed LDS reads.
// Slab per workgroup: [TAIL_TILES][16][64]; layout in packing.ends_grad_tables.
// ---------------------------------------------------------------------------------------------

template <typename T, int F, int R, int LOSS = 0>
__global__ __launch_bounds__(896) void sr_tail_wgrad_kernel(const float* __restrict__ dout, const T* __restrict__ feat,
                                                            const float* __restrict__ ximg, float mean,
                                                            float* __restrict__ partial, int N, int H, int W,
                                                            int tiles_x, int tiles_per_img, LossIn li, float* __restrict__ loss_part) {
  typedef EndsCfg<F, R> E;
  typedef typename E::template Img<2> I;
  typedef typename FragOf<T>::type FragT;
  constexpr int NT = E::NT, NTHREADS = 896;
  __shared__ __attribute__((aligned(16))) T smem[E::DCC_ELEMS + E::FT_ELEMS + I::ELEMS];
  T* const DC = smem;
  T* const FT = DC + E::DCC_ELEMS;
  T* const XI = FT + E::FT_ELEMS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool is_tap = wave < 9;
  const int ty = is_tap ? wave / 3 : wave - 9, tx = is_tap ? wave % 3 : 0;

  f32x16 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) acc[i] = zero16();
  float lsum = 0.f;

  SR_STAMP_DECL;
  SR_STAMP();
  for (int t = blockIdx.x; t < N * tiles_per_img; t += gridDim.x) {
    const int n = t / tiles_per_img, tile = t - n * tiles_per_img;
    const int ty0 = (tile / tiles_x) * E::TH, tx0 = (tile % tiles_x) * E::TW;
    __syncthreads();
    SR_STAMP();
    LossIn lin = li;
    lin.hr += LOSS ? (size_t)n * 3 * H * R * W * R : 0;
    stage_dconv<T, E, 0, NTHREADS, LOSS>(DC, dout + (size_t)n * 3 * H * R * W * R, H, W, ty0, tx0, tid, lin, &lsum);
    SR_STAMP();
    stage_halo<T, E, F, NTHREADS>(FT, feat + (size_t)n * H * W * F, H, W, ty0, tx0, tid);
    stage_img<T, E, 2, NTHREADS>(XI, ximg + (size_t)n * 3 * H * W, mean, H, W, ty0, tx0, tid);
    SR_STAMP();
    __syncthreads();
    SR_STAMP();
    constexpr int UNR = sizeof(T) == 2 ? 3 : 1;
#pragma unroll UNR
    for (int ot = 0; ot < E::NPT_O; ++ot) {
      const int toy = (ot / (E::TW / 8)) * 4, tox = (ot % (E::TW / 8)) * 8;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        FragT b;
        if (is_tap) b = tr_frag<T>(FT, s, lane, [=](int p) { return ((toy + (p >> 3) + ty) * E::HW + tox + (p & 7) + tx) * F; });
        else b = tr_frag<T>(XI, s, lane, [=](int p) { return ((toy + (p >> 3) + ty) * I::IW + tox + (p & 7)) * 4; });
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) {
          const FragT a = tr_frag<T>(DC, s, lane, [=](int p) { return ((toy + (p >> 3)) * E::TW + tox + (p & 7)) * E::COP + 32 * ti; });
          acc[ti] = mma16<T>(a, b, acc[ti]);
        }
      }
    }
  }
  SR_STAMP();
  // global tile index: taps (ty*3 + tx)*NT + ti ; skip rows 9*NT + ky*NT + ti
  float* out = partial + (size_t)blockIdx.x * E::TAIL_TILES * 1024;
  const int gbase = is_tap ? (ty * 3 + tx) * NT : (9 + ty) * NT;
#pragma unroll
  for (int ti = 0; ti < NT; ++ti)
#pragma unroll
    for (int i = 0; i < 16; ++i) out[((gbase + ti) * 16 + i) * 64 + lane] = acc[ti][i];
  if constexpr (LOSS != 0) wg_sum_store<NTHREADS>(lsum, reinterpret_cast<float*>(smem), loss_part + blockIdx.x, tid);
  SR_STAMP();
}

// ---------------------------------------------------------------------------------------------
// head weight gradient: tiles [ky] = [f rows, (kx, ci) columns], dy0 = gradient w.r.t. the head output.
// 9 waves: wave (ky, grp) owns tile ky over the pixel tiles grp, grp+3, grp+6.
// ---------------------------------------------------------------------------------------------
template <typename T, int F>
__global__ __launch_bounds__(576) void sr_head_wgrad_kernel(const T* __restrict__ dy0, const float* __restrict__ ximg,
                                                            float mean, float* __restrict__ partial, int N, int H,
                                                            int W, int tiles_x, int tiles_per_img) {
  typedef EndsCfg<F, 4> E;
  typedef typename E::template Img<1> I;
  typedef typename FragOf<T>::type FragT;
  constexpr int NTHREADS = 576;
  constexpr int STAGE_BYTES = (E::DYC_ELEMS + I::ELEMS) * (int)sizeof(T);
  constexpr int SLAB_BYTES = 9 * 1024 * 4;
  constexpr int LDS_BYTES = STAGE_BYTES > SLAB_BYTES ? STAGE_BYTES : SLAB_BYTES;
  __shared__ __attribute__((aligned(16))) char smem_raw[LDS_BYTES];
  T* const DY = reinterpret_cast<T*>(smem_raw);
  T* const XI = DY + E::DYC_ELEMS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ky = wave / 3, grp = wave - ky * 3;
  f32x16 acc = zero16();
  for (int t = blockIdx.x; t < N * tiles_per_img; t += gridDim.x) {
    const int n = t / tiles_per_img, tile = t - n * tiles_per_img;
    const int ty0 = (tile / tiles_x) * E::TH, tx0 = (tile % tiles_x) * E::TW;
    __syncthreads();
    stage_core<T, E, F, NTHREADS>(DY, dy0 + (size_t)n * H * W * F, H, W, ty0, tx0, tid);
    stage_img<T, E, 1, NTHREADS>(XI, ximg + (size_t)n * 3 * H * W, mean, H, W, ty0, tx0, tid);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int ot = grp + 3 * k;
      const int toy = (ot / (E::TW / 8)) * 4, tox = (ot % (E::TW / 8)) * 8;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const FragT a = tr_frag<T>(DY, s, lane, [=](int p) { return ((toy + (p >> 3)) * E::TW + tox + (p & 7)) * F; });
        const FragT b = tr_frag<T>(XI, s, lane, [=](int p) { return ((toy + (p >> 3) + ky) * I::IW + tox + (p & 7)) * 4; });
        acc = mma16<T>(a, b, acc);
      }
    }
  }
  __syncthreads();
  float* slab = reinterpret_cast<float*>(smem_raw);           // [ky][grp][1024]: plain stores, no LDS atomics
  slab_store_tile(slab, wave, acc, lane);
  __syncthreads();
  float* out = partial + (size_t)blockIdx.x * 3 * 1024;
  for (int i = tid; i < 3 * 1024; i += NTHREADS) {
    const int k = i >> 10, w = i & 1023;
    out[i] = slab[(3 * k) * 1024 + w] + slab[(3 * k + 1) * 1024 + w] + slab[(3 * k + 2) * 1024 + w];
  }
}

// ---------------------------------------------------------------------------------------------
// The two phases of the fused tail backward over one tile whose dconv image (with halo) is in LDS, as functions, for
// sr_tail_train_kernel.  (sr_tail_bwd_kernel below keeps its own text of the same loops: built on these functions, two of
// its instantiations need one register more than a wave has, and the build refuses a spill.)
// ---------------------------------------------------------------------------------------------
// dfeat[px, f] = sum_{u, ch} Wt[ch, f, 8-u] dconv[px + u - 1, ch] for the 32-pixel output tile `ot` (one wave)
template <typename T, typename E, int UNRD, typename WS>
SR_DEV void tail_dfeat_tile(const T* DC, const WS& wsrc, T* __restrict__ dfeat, int n, int H, int W, int ty0, int tx0, int ot, int lane) {
  typedef typename FragOf<T>::half_type HalfT;
  const int r = lane & 31, hh = lane >> 5;
  const int oy = (ot / (E::TW / 8)) * 4 + (r >> 3), ox = (ot % (E::TW / 8)) * 8 + (r & 7);
  const int hbase = oy * E::HW + ox;
  f32x16 d = zero16();
#pragma unroll UNRD
  for (int s = 0; s < E::KSTB; ++s) {
    const int q = 2 * s + hh;
    int off = hbase * E::COP;
    if (q < 9 * E::CC) {
      const int u = q / E::CC, c = q - u * E::CC;
      off = (hbase + (u / 3) * E::HW + (u % 3)) * E::COP + c * 8;
    }
    d = mma16<T>(wsrc.get(s, lane), lds_chunk<T>(DC, off), d);
  }
  const int Y = ty0 + oy, X = tx0 + ox;
  if (Y < H && X < W) {
    T* o = dfeat + (((size_t)n * H + Y) * W + X) * E::F;
#pragma unroll
    for (int g = 0; g < E::FC; ++g) stream_store(reinterpret_cast<HalfT*>(o + g * 8 + hh * 4), acc_group<T>(d, g));
  }
}
// this wave's weight-gradient tiles (tap (ty, tx) of the 3x3 conv, or skip row ty) over the nine pixel tiles of the tile.
// FT is read as the feature tile with a 1-px halo and XI as x - mean with a 2-px halo; PF / PX are the halos the two LDS
// images were STAGED with (PF >= 1, PX >= 2): a wider image is read through its row stride, from the pointer to its pixel
// (PF - 1, PF - 1) resp. (PX - 2, PX - 2) (tail_view_origin) -- no narrow copy.  One transposed read covers eight pixels of one
// image row, so the row stride does not enter its bank pattern.
template <typename E, int PF, int PX> struct tail_view_origin {
  static constexpr int FT = (PF - 1) * (E::TW + 2 * PF + 1) * E::F, XI = (PX - 2) * (E::template Img<PX>::IW + 1) * 4;   // elements
};
template <typename T, typename E, int UNR, int PF = 1, int PX = 2>
SR_DEV void tail_wgrad_tile(const T* DC, const T* FT, const T* XI, f32x16 (&acc)[E::NT], bool is_tap, int ty, int tx, int lane) {
  typedef typename E::template Img<PX> I;
  typedef typename FragOf<T>::type FragT;
  constexpr int FW_ = E::TW + 2 * PF;                           // the feature image's row stride, in pixels
#pragma unroll UNR
  for (int ot = 0; ot < E::NPT_O; ++ot) {
    const int toy = (ot / (E::TW / 8)) * 4, tox = (ot % (E::TW / 8)) * 8;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      FragT b;
      if (is_tap) b = tr_frag<T>(FT, s, lane, [=](int p) { return ((toy + (p >> 3) + ty) * FW_ + tox + (p & 7) + tx) * E::F; });
      else b = tr_frag<T>(XI, s, lane, [=](int p) { return ((toy + (p >> 3) + ty) * I::IW + tox + (p & 7)) * 4; });
#pragma unroll
      for (int ti = 0; ti < E::NT; ++ti) {
        const FragT a = tr_frag<T>(DC, s, lane, [=](int p) { return ((toy + (p >> 3) + 1) * E::HW + tox + (p & 7) + 1) * E::COP + 32 * ti; });
        acc[ti] = mma16<T>(a, b, acc[ti]);
      }
    }
  }
}
// the wave's accumulator tiles into the workgroup's slab: taps (ty*3 + tx)*NT + ti ; skip rows 9*NT + ky*NT + ti
template <typename E>
SR_DEV void tail_slab_store(float* __restrict__ partial, const f32x16 (&acc)[E::NT], bool is_tap, int ty, int tx, int lane) {
  float* out = partial + (size_t)blockIdx.x * E::TAIL_TILES * 1024;
  const int gbase = is_tap ? (ty * 3 + tx) * E::NT : (9 + ty) * E::NT;
#pragma unroll
  for (int ti = 0; ti < E::NT; ++ti)
#pragma unroll
    for (int i = 0; i < 16; ++i) out[((gbase + ti) * 16 + i) * 64 + lane] = acc[ti][i];
}
// unroll factors of the two phases (bf16, 128-register budget)
template <typename E, int LOSS> struct TailBwdUnroll {
  static constexpr int UNRD = (E::NT > 1 && E::F > 24) ? 3 : E::KSTB;      // x4 / 32 units: keep the operand prefetch short
  static constexpr int UNR = (E::NT > 1 || (LOSS != 0 && E::R == 2)) ? 1 : 3;   // x4: two accumulator tiles per wave
};

// ---------------------------------------------------------------------------------------------
// tail backward, data and weight gradients in one launch (bf16): both stage the same un-shuffled HR gradient
// tile (14 MB of fp32 per batch), so the fused kernel reads it once and drops a dependent launch.  Per tile
// waves 0..8 first compute dfeat for one 32-pixel tile each (weights staged once per workgroup in LDS), then all
// 14 waves accumulate their weight-gradient tiles as sr_tail_wgrad_kernel does (no barrier in between: both
// only read LDS).  Bit-identical to sr_tail_bwd_data_kernel + sr_tail_wgrad_kernel with the same grid.
// ---------------------------------------------------------------------------------------------
template <typename T, int F, int R, int LOSS = 0>
__global__ __launch_bounds__(896) void sr_tail_bwd_kernel(const float* __restrict__ dout, const T* __restrict__ feat,
                                                          const float* __restrict__ ximg, float mean,
                                                          const T* __restrict__ wblob, T* __restrict__ dfeat,
                                                          float* __restrict__ partial, int N, int H, int W, int tiles_x,
                                                          int tiles_per_img, LossIn li, float* __restrict__ loss_part) {
  typedef EndsCfg<F, R> E;
  typedef typename E::template Img<2> I;
  typedef typename FragOf<T>::type FragT;
  typedef typename FragOf<T>::half_type HalfT;
  static_assert(sizeof(T) == 2, "bf16 only");
  constexpr int NT = E::NT, NTHREADS = 896;
  __shared__ __attribute__((aligned(16))) T smem[E::DC_ELEMS + E::FT_ELEMS + I::ELEMS + E::KSTB * 512];
  T* const DC = smem;                       // dconv with halo [NPXH_PAD + 2][COP]
  T* const FT = DC + E::DC_ELEMS;
  T* const XI = FT + E::FT_ELEMS;
  T* const WL = XI + I::ELEMS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const bool is_tap = wave < 9;
  const int ty = is_tap ? wave / 3 : wave - 9, tx = is_tap ? wave % 3 : 0;
  stage_weights<T, NTHREADS>(WL, wblob + (size_t)E::NT * E::KST * 512, E::KSTB, tid);   // backward-data section
  WSrc<T, true> wsrc;
  wsrc.p = WL;

  f32x16 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) acc[i] = zero16();
  __shared__ float lsum_lds[LOSS ? NTHREADS : 1];      // this thread's loss partial lives in LDS: no VGPR to spare here
  if constexpr (LOSS != 0) lsum_lds[tid] = 0.f;

  for (int t = blockIdx.x; t < N * tiles_per_img; t += gridDim.x) {
    const int n = t / tiles_per_img, tile = t - n * tiles_per_img;
    const int ty0 = (tile / tiles_x) * E::TH, tx0 = (tile % tiles_x) * E::TW;
    __syncthreads();
    LossIn lin = li;
    lin.hr += LOSS ? (size_t)n * 3 * H * R * W * R : 0;
    {
      float lsum = 0.f;
      stage_dconv<T, E, 1, NTHREADS, LOSS>(DC, dout + (size_t)n * 3 * H * R * W * R, H, W, ty0, tx0, tid, lin, &lsum);
      if constexpr (LOSS != 0) lsum_lds[tid] += lsum;
    }
    stage_halo<T, E, F, NTHREADS>(FT, feat + (size_t)n * H * W * F, H, W, ty0, tx0, tid);
    stage_img<T, E, 2, NTHREADS>(XI, ximg + (size_t)n * 3 * H * W, mean, H, W, ty0, tx0, tid);
    __syncthreads();
    if (wave < E::NPT_O) {                  // dfeat[px, f] = sum_{u, ch} Wt[ch, f, 8-u] dconv[px + u - 1, ch]
      const int ot = wave;
      const int oy = (ot / (E::TW / 8)) * 4 + (r >> 3), ox = (ot % (E::TW / 8)) * 8 + (r & 7);
      const int hbase = oy * E::HW + ox;
      f32x16 d = zero16();
      constexpr int UNRD = (NT > 1 && F > 24) ? 3 : E::KSTB;      // x4 / 32 units: keep the operand prefetch short
#pragma unroll UNRD
      for (int s = 0; s < E::KSTB; ++s) {
        const int q = 2 * s + hh;
        int off = hbase * E::COP;
        if (q < 9 * E::CC) {
          const int u = q / E::CC, c = q - u * E::CC;
          off = (hbase + (u / 3) * E::HW + (u % 3)) * E::COP + c * 8;
        }
        d = mma16<T>(wsrc.get(s, lane), lds_chunk<T>(DC, off), d);
      }
      const int Y = ty0 + oy, X = tx0 + ox;
      if (Y < H && X < W) {
        T* o = dfeat + (((size_t)n * H + Y) * W + X) * F;
#pragma unroll
        for (int g = 0; g < E::FC; ++g) stream_store(reinterpret_cast<HalfT*>(o + g * 8 + hh * 4), acc_group<T>(d, g));
      }
    }
    // x4: two accumulator tiles per wave, 128-register budget; x3 / 32 units sits on that budget's edge (one register over
    // or not with the kernels around it in the translation unit), so it takes the short form too
    constexpr int UNR = (NT > 1 || (LOSS != 0 && R == 2) || (R == 3 && F > 24)) ? 1 : 3;
#pragma unroll UNR
    for (int ot = 0; ot < E::NPT_O; ++ot) {
      const int toy = (ot / (E::TW / 8)) * 4, tox = (ot % (E::TW / 8)) * 8;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        FragT b;
        if (is_tap) b = tr_frag<T>(FT, s, lane, [=](int p) { return ((toy + (p >> 3) + ty) * E::HW + tox + (p & 7) + tx) * F; });
        else b = tr_frag<T>(XI, s, lane, [=](int p) { return ((toy + (p >> 3) + ty) * I::IW + tox + (p & 7)) * 4; });
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) {
          const FragT a = tr_frag<T>(DC, s, lane, [=](int p) { return ((toy + (p >> 3) + 1) * E::HW + tox + (p & 7) + 1) * E::COP + 32 * ti; });
          acc[ti] = mma16<T>(a, b, acc[ti]);
        }
      }
    }
  }
  float* out = partial + (size_t)blockIdx.x * E::TAIL_TILES * 1024;
  const int gbase = is_tap ? (ty * 3 + tx) * NT : (9 + ty) * NT;
#pragma unroll
  for (int ti = 0; ti < NT; ++ti)
#pragma unroll
    for (int i = 0; i < 16; ++i) out[((gbase + ti) * 16 + i) * 64 + lane] = acc[ti][i];
  if constexpr (LOSS != 0) wg_sum_store<NTHREADS>(lsum_lds[tid], reinterpret_cast<float*>(smem), loss_part + blockIdx.x, tid);
}

// ---------------------------------------------------------------------------------------------
// tail forward + loss + tail backward in one launch (the training step; bf16, R = 4, LOSS 1 / 2): the SR image only
// ever exists in the accumulators.  Same grid, workgroup and tile walk as sr_tail_bwd_kernel<.., LOSS>.  Per tile
//   1. stage every operand ONCE: the forward's weight fragments, feat with a 2-px halo and x - mean with a 3-px halo.  The
//      backward phases read feat with a 1-px halo and x - mean with a 2-px halo: sub-windows of the same two LDS images,
//      reached through their row stride and origin (tail_wgrad_tile<.., PF = 2, PX = 3>, tail_view_origin), not staged again;
//   2. waves 0..11 compute conv3x3 + skip + constants for one 32-pixel tile each of the core tile AND its 1-px halo
//      (14 x 26 = 364 pixels), k-steps and operands exactly as sr_tail_fwd_kernel's, so the accumulator holds the fp32
//      value that kernel would have stored;
//   3. loss_grad<LOSS> against hr straight from the accumulator -> the bf16 dconv image with halo (zero outside the
//      image); the fp32 loss terms of the core pixels go to LDS (both over the forward's operands, dead by then) ...
//   4. ... where the thread that owns an HR row of four in stage_dconv's order adds them up, so the per-thread fp32 sums,
//      and with them loss_part, come out bit for bit as sr_tail_bwd_kernel<.., LOSS> forms them;
//   5. the dfeat and weight-gradient phases of sr_tail_bwd_kernel, unchanged.
// Bit-identical to sr_tail_fwd_kernel + sr_tail_bwd_kernel<.., LOSS> with the same grid.
//
// ONE = the launch gives every workgroup at most one tile (gridDim.x >= N * tiles_per_img; the training step at batch <= 32
// of 48 x 48 patches): no tile loop, so both weight sections and both images go out in one burst with one barrier before the
// first MFMA, the per-thread loss sum stays in a register, and the lane's index arithmetic is plain code (84 VGPRs).  With the loop
// (!ONE) that arithmetic is re-derived per tile from laundered ids (tile_local), since hoisted out of the loop it would sit
// in registers past the 128 a wave has here, and the forward's weights are staged again per tile, dconv having overwritten them.
//
// LDS map (bf16 elements; F = 24 / 32), 145888 / 153056 bytes (+ 3584 with the loop) of the 163840 a workgroup may take:
//   FT2  [(TH + 4)(TW + 4)][F]   feat, 2-px halo            10752 / 14336   live from staging to the last weight-gradient read
//   XI3  [Img<3>::ELEMS]         x - mean | 1, 3-px halo     2192            (directly behind FT2: the forward addresses both from FT2)
//   WL   [KSTB][512]             backward-data weights      13824
//   U    one region, a barrier between its two uses:                        46176
//          FW [NT KST][512]      forward weights            21504 / 26624   dead after the forward products
//          DC [NPXH_PAD + 2][COP] dconv, 1-px halo          18528           + TERM [NPXC][CO] fp32 loss terms 27648
//   lsum_lds [896] fp32 (!ONE only): the per-thread loss sums across tiles
// ---------------------------------------------------------------------------------------------
// `v` as the compiler may not carry it across tiles (see above); the identity where there is no tile loop
template <bool ONE> SR_DEV int tile_local(int v) {
  if constexpr (!ONE) asm volatile("" : "+v"(v));
  return v;
}
template <typename T, int F, int R, int LOSS, bool ONE>
__global__ __launch_bounds__(896) void sr_tail_train_kernel(const T* __restrict__ feat, const float* __restrict__ ximg, float mean,
                                                            const T* __restrict__ wblob, T* __restrict__ dfeat,
                                                            float* __restrict__ partial, int N, int H, int W, int tiles_x,
                                                            int tiles_per_img, LossIn li, float* __restrict__ loss_part) {
  typedef EndsCfg<F, R> E;
  typedef typename E::template Img<3> I3;
  typedef typename FragOf<T>::type FragT;
  typedef typename FragOf<T>::half_type HalfT;
  static_assert(sizeof(T) == 2 && R == 4 && LOSS != 0 && E::COP == E::CO, "bf16, x4, with the loss");
  constexpr int NT = E::NT, NTHREADS = 896;
  constexpr int NPT_H = E::NPXH_PAD / 32;                          // forward pixel tiles over the halo'd tile: one wave each
  static_assert(NPT_H * 64 <= NTHREADS, "one wave per forward pixel tile");
  constexpr int HW2 = E::TW + 4, NPX2 = HW2 * (E::TH + 4);         // feat with a 2-px halo
  constexpr int FT2_ELEMS = NPX2 * F, FW_ELEMS = NT * E::KST * 512;
  constexpr int TERM_ELEMS = E::NPXC * E::CO * 2;                  // fp32 loss terms [core px][CO], in units of T
  constexpr int BWD_ELEMS = E::DC_ELEMS + TERM_ELEMS;              // what the forward leaves behind: the dconv image and the loss terms
  constexpr int U_ELEMS = FW_ELEMS > BWD_ELEMS ? FW_ELEMS : BWD_ELEMS;   // one region for both, a barrier in between
  constexpr int LDS_ELEMS = FT2_ELEMS + I3::ELEMS + E::KSTB * 512 + U_ELEMS;
  constexpr int NLSUM = ONE ? 1 : NTHREADS;
  static_assert(LDS_ELEMS * sizeof(T) + NLSUM * sizeof(float) <= 160 * 1024, "the LDS a workgroup may take");
  static_assert(FT2_ELEMS % 8 == 0 && I3::ELEMS % 8 == 0, "16-byte aligned regions");
  __shared__ __attribute__((aligned(16))) T smem[LDS_ELEMS];
  T* const FT2 = smem;                      // feat with a 2-px halo; x - mean with a 3-px halo follows
  constexpr int XI3_0 = FT2_ELEMS;
  T* const WL = FT2 + FT2_ELEMS + I3::ELEMS;
  T* const DC = WL + E::KSTB * 512;         // dconv with halo [NPXH_PAD + 2][COP]
  float* const TERM = reinterpret_cast<float*>(DC + E::DC_ELEMS);
  T* const FW = DC;                         // forward section of the weight blob
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const bool is_tap = wave < 9;
  const int ty = is_tap ? wave / 3 : wave - 9, tx = is_tap ? wave % 3 : 0;
  stage_weights<T, NTHREADS>(WL, wblob + (size_t)E::NT * E::KST * 512, E::KSTB, tid);   // backward-data section
  WSrc<T, true> wsrc, wfwd;
  wsrc.p = WL;
  wfwd.p = FW;

  f32x16 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) acc[i] = zero16();
  __shared__ float lsum_lds[NLSUM];         // with the loop this thread's loss partial lives in LDS: no VGPR to spare there
  float lsum_one = 0.f;
  if constexpr (!ONE) lsum_lds[tid] = 0.f;
  SR_STAMP_DECL;
  SR_STAMP();                               // kernel entry

  // forward: this lane's pixel of the halo'd tile (row p of the dconv image)
  const int p = wave * 32 + r;
  const bool fwd_wave = wave < NPT_H;
  constexpr int NG = E::CO / 8;                                    // groups of four conv channels per lane half: one HR row of four each

  for (int t = blockIdx.x; t < N * tiles_per_img; t += gridDim.x) {
    const int n = t / tiles_per_img, tile = t - n * tiles_per_img;
    const int ty0 = (tile / tiles_x) * E::TH, tx0 = (tile % tiles_x) * E::TW;
    const int p_t = tile_local<ONE>(p);
    const int pp = (fwd_wave && p_t < E::NPXH) ? p_t : 0;
    const int py = pp / E::HW, px = pp - py * E::HW;
    const bool core = py >= 1 && py <= E::TH && px >= 1 && px <= E::TW;
    const int Y = ty0 - 1 + py, X = tx0 - 1 + px;
    const bool live = fwd_wave && p < E::NPXH && Y >= 0 && Y < H && X >= 0 && X < W;
    const float* const hr = li.hr + (size_t)n * 3 * H * R * W * R;
    // The target's values for this lane's accumulator rows: NG HR rows of four.  Holding them from here would cost 4 NG
    // registers through the products (with the tile loop there are none to spare; without it there are, and it was measured:
    // 0.7 us of 21.5, inside the run-to-run spread, not kept), so one float of each row is read now, which brings the
    // rows' cache lines in under the staging and the products, and the rows themselves are read after the products.
    const unsigned hrw = (unsigned)W * R, plane = (unsigned)H * R * hrw;
    const unsigned hoff = ((unsigned)Y * R) * hrw + (unsigned)X * R + (hh ? hrw : 0u);   // row si = hh of colour 0
    float touch = 0.f;
    if (live) {
#pragma unroll
      for (int k = 0; k < NG; ++k) touch += hr[hoff + (k >> 1) * plane + (k & 1) * 2 * hrw];
    }
    if constexpr (!ONE) __syncthreads();    // the previous tile's backward phases are through with the images and DC
    const int tid_t = tile_local<ONE>(tid);
    stage_weights<T, NTHREADS>(FW, wblob, NT * E::KST, tid);
    stage_rows<T, F, HW2, NPX2, NPX2, NTHREADS>(FT2, feat + (size_t)n * H * W * F, H, W, ty0 - 2, tx0 - 2, tid_t);
    stage_img<T, E, 3, NTHREADS>(FT2 + XI3_0, ximg + (size_t)n * 3 * H * W, mean, H, W, ty0, tx0, tid_t);
    __syncthreads();
    SR_STAMP();                             // operands staged
    f32x16 facc[NT];
    if (fwd_wave) {                         // out^T tile = conv3x3 + skip + constants, as sr_tail_fwd_kernel forms it
      const int lane_f = tile_local<ONE>(lane);
      const int hh_f = lane_f >> 5, hbase = py * HW2 + px;
#pragma unroll
      for (int ti = 0; ti < NT; ++ti) facc[ti] = zero16();
      const int fbase = hbase * F, xbase = XI3_0 + (py * I3::IW + px) * 4;
      // LDS offset of operand chunk q (sr_tail_fwd_kernel's order: nine taps x FC feature chunks, then 15 skip chunks of two
      // pixels, the rest on zero weights); q is a constant once unrolled, the lane half picks one of two
      auto chunk_off = [&](int q) {
        if (q < 9 * E::FC) {
          const int tap = q / E::FC, c = q - tap * E::FC;
          return fbase + ((tap / 3) * HW2 + (tap % 3)) * F + c * 8;
        }
        int qs = q - 9 * E::FC;
        if (qs >= 15) qs = 0;                                 // zero weights there
        const int ky = qs / 3, m = qs - ky * 3;
        return xbase + (ky * I3::IW + 2 * m) * 4;
      };
#pragma unroll
      for (int s = 0; s < E::KST; ++s) {
        const int off = hh_f ? chunk_off(2 * s + 1) : chunk_off(2 * s);
        const FragT b = 2 * s + 1 < 9 * E::FC ? lds_chunk<T>(FT2, off) : lds_chunk_half<T>(FT2, off);
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) facc[ti] = mma16<T>(wfwd.get(ti * E::KST + s, lane_f), b, facc[ti]);
      }
    }
    SR_STAMP();                             // forward products
    asm volatile("" :: "v"(touch));
    f32x4 hv[NG];
    if (live) {
#pragma unroll
      for (int k = 0; k < NG; ++k)          // rows ch0 = 8 k + 4 hh: colour k >> 1, sub-row 2 (k & 1) + hh
        hv[k] = *reinterpret_cast<const f32x4*>(hr + (hoff + (k >> 1) * plane + (k & 1) * 2 * hrw));
    } else {
#pragma unroll
      for (int k = 0; k < NG; ++k) hv[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();                        // the forward's operands are dead: the loss terms take their place
    if (fwd_wave) {
#pragma unroll
      for (int k = 0; k < NG; ++k) {
        const int ti = k >> 2, g = k & 3, ch0 = 8 * k + 4 * hh;   // rows ch0 .. ch0+3 live in regs 4g..4g+3 of tile ti
        HalfT dv;
        f32x4 tv;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float term = 0.f;
          const float gj = live ? loss_grad<LOSS>(facc[ti][4 * g + j], hv[k][j], li.gscale, term) : 0.f;
          dv[j] = (T)gj;
          tv[j] = term;
        }
        *reinterpret_cast<HalfT*>(DC + p * E::COP + ch0) = dv;
        if (live && core) *reinterpret_cast<f32x4*>(TERM + ((py - 1) * E::TW + px - 1) * E::CO + ch0) = tv;
      }
    } else if (wave == NPT_H) {             // the two spare rows of the dconv image
      constexpr int NCH = 2 * E::COP / 8;
      FragT z;
#pragma unroll
      for (int j = 0; j < 8; ++j) z[j] = (T)0.f;
      if (lane < NCH) *reinterpret_cast<FragT*>(DC + E::NPXH_PAD * E::COP + lane * 8) = z;
    }
    __syncthreads();
    SR_STAMP();                             // dconv and the loss terms in LDS
    {                                       // loss terms of the core pixels, each added by its owner in stage_dconv's order
      constexpr int ROWS = 3 * R, TOTAL = (E::NPXH_PAD + 2) * ROWS, ITER = (TOTAL + NTHREADS - 1) / NTHREADS;
      float lsum = 0.f;
      const int tid_l = tile_local<ONE>(tid);
#pragma unroll
      for (int it = 0; it < ITER; ++it) {
        const int idx = tid_l + it * NTHREADS;
        const int q = idx / ROWS, cr = idx - q * ROWS;
        if (q < E::NPXH) {
          const int qy = q / E::HW, qx = q - qy * E::HW;
          if (qy >= 1 && qy <= E::TH && qx >= 1 && qx <= E::TW && ty0 - 1 + qy < H && tx0 - 1 + qx < W) {
            const f32x4 tv = *reinterpret_cast<const f32x4*>(TERM + ((qy - 1) * E::TW + qx - 1) * E::CO + cr * R);
#pragma unroll
            for (int j = 0; j < R; ++j) lsum += tv[j];
          }
        }
      }
      if constexpr (ONE) lsum_one = lsum;
      else lsum_lds[tid] += lsum;
    }
    typedef TailBwdUnroll<E, LOSS> U;
    const int lane_d = tile_local<ONE>(lane);
    if (wave < E::NPT_O) tail_dfeat_tile<T, E, U::UNRD>(DC, wsrc, dfeat, n, H, W, ty0, tx0, wave, lane_d);
    SR_STAMP();                             // loss sums and dfeat
    typedef tail_view_origin<E, 2, 3> V;
    tail_wgrad_tile<T, E, U::UNR, 2, 3>(DC, FT2 + V::FT, FT2 + XI3_0 + V::XI, acc, is_tap, ty, tx, lane_d);
    SR_STAMP();                             // weight-gradient products
    if constexpr (ONE) break;               // gridDim.x >= N * tiles_per_img: there is no second tile
  }
  tail_slab_store<E>(partial, acc, is_tap, ty, tx, lane);
  wg_sum_store<NTHREADS>(ONE ? lsum_one : lsum_lds[ONE ? 0 : tid], reinterpret_cast<float*>(smem), loss_part + blockIdx.x, tid);
  SR_STAMP();                               // slab and loss_part written
}
