// Searched-network (Result_Model) kernels, gfx950: the k x k residual conv on a channel window of the NAS stage-3 trainer
// (reference: pretrain_simplified_model.py Block / Conv_sep(seperate=False)), its backward, and the k x k tail conv
// (k in {5, 7}) that the reference builds with the last block's kernel size.
//
// Everything here is one implicit-GEMM shape on v_mfma_f32_32x32x16_bf16 (fp32 parity mode: 8 x v_mfma_f32_32x32x2_f32 per
// k-step, sr_common.h):
//   * rm_conv_kernel:  D[out channel][pixel] = sum_{tap, ci} Wp[out channel][(tap, ci)] * in[pixel + tap][ci]
//     A = packed weights (rows = output channels, 32 per row tile, k = tap * CI + ci, zero past K*K*CI), read from global
//     memory (L2) once per k-step and wave and used for RPW pixel tiles; B = 8 consecutive channels of one staged pixel
//     (CI is a multiple of 8, so a B chunk never straddles a tap).  The input tile (TH + 2P) x (TW + 2P) sits in LDS with
//     a pixel stride of an odd number of 16-byte slots (conflict-free ds_read_b128 over consecutive pixels).
//     Epilogues: EP_BLOCK  y = x + ReLU(acc + b), packed ReLU mask (bit c of a uint32 per pixel = z_c > 0)
//                EP_BWD    dx = dy + acc, the input staged as dy * mask (the forward's saved bits, never y - x)
//                EP_STORE  y = acc (tail backward-data into the feature gradient)
//                EP_MSTORE y = acc, the input staged as dy * mask as for EP_BWD, no residual (a backward-data branch that does not
//                          carry the block's skip: the multi-frame network's warp group)
//                EP_SHUF   out[n][c][R y + i][R x + j] += acc[c R^2 + i R + j] (tail forward: PixelShuffle as addressing,
//                          added onto the skip + bias output of sr_tail_fwd run with zero 3x3 weights)
//   * rm_wgrad_kernel: D[out channel][ci] of tap t = sum_p g[p][out channel] * in[p + tap][ci], plus one bias tile
//     (B = ones).  Both operands are transposed LDS reads (tr_frag, 16 pixels per k-step); every workgroup walks
//     16 x 16 pixel tiles of all images and writes one fp32 slab per (tile group, workgroup); the host sums the slabs.
// Block weights are embedded in the F-channel row: rows / columns outside the window [IN - split, IN) are zero, so the
// pass-through and padded channels get acc = 0, ReLU(0) = 0 and are copied bit for bit.
#pragma once
#include "sr_common.h"

enum { RM_EP_BLOCK = 0, RM_EP_BWD = 1, RM_EP_STORE = 2, RM_EP_SHUF = 3, RM_EP_MSTORE = 4 };

template <typename T, int K, int CI, int COUT>
struct RmConvCfg {
  static constexpr int P = K / 2, TW = 32, TH = sizeof(T) == 2 ? 16 : 8, NW = 4, RPW = TH / NW;
  static constexpr int SW = TW + 2 * P, SH = TH + 2 * P, NPIX = SW * SH;
  static constexpr int CS = ((CI / 8) & 1) ? CI : CI + 8;          // LDS pixel stride: odd number of 16-byte slots
  static constexpr int KS = (K * K * CI + 15) / 16, NRT = (COUT + 31) / 32;
  static constexpr int LDS_BYTES = NPIX * CS * (int)sizeof(T);
};

// NHWC tile with a P-pixel halo -> LDS [pixel][CS], zero outside the image; MASK: channel c kept iff bit c of mask[pixel]
template <typename T, int CI, int CS, int SW, int NPIX, bool MASK, int NTHREADS>
SR_DEV void rm_stage(T* dst, const T* __restrict__ src, const uint32_t* __restrict__ mask, int H, int W, int y0, int x0,
                     int tid) {
  typedef typename FragOf<T>::type FragT;
  constexpr int NC = CI / 8, TOTAL = NPIX * NC;
  for (int idx = tid; idx < TOTAL; idx += NTHREADS) {
    const int p = idx / NC, c = idx - p * NC;
    const int py = p / SW, px = p - py * SW;
    const int Y = y0 + py, X = x0 + px;
    FragT v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (T)0.f;
    if (Y >= 0 && Y < H && X >= 0 && X < W) {
      const size_t pix = (size_t)Y * W + X;
      v = *reinterpret_cast<const FragT*>(src + pix * CI + c * 8);
      if constexpr (MASK) {
        const uint32_t m = mask[pix] >> (c * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (!((m >> j) & 1u)) v[j] = (T)0.f;
      }
    }
    *reinterpret_cast<FragT*>(dst + p * CS + c * 8) = v;
  }
}

// in / res / out are the n-th image's base pointers (NHWC, CI resp. COUT channels); wp: NRT x KS packed fragments;
// bias (EP_BLOCK): float[32]; mask: uint32 per pixel (EP_BLOCK writes it, EP_BWD and EP_MSTORE read it); hr (EP_SHUF): NCHW fp32
template <typename T, int K, int CI, int COUT, int EP, int R>
__global__ void __launch_bounds__(256) rm_conv_kernel(const T* __restrict__ in, const T* __restrict__ res, T* __restrict__ out,
                                                      float* __restrict__ hr, const T* __restrict__ wp,
                                                      const float* __restrict__ bias, uint32_t* __restrict__ mask, int H,
                                                      int W, int tiles_x) {
  typedef RmConvCfg<T, K, CI, COUT> C;
  typedef typename FragOf<T>::type FragT;
  typedef typename FragOf<T>::half_type HalfT;
  __shared__ __attribute__((aligned(16))) unsigned char rm_smem[C::LDS_BYTES];
  T* tile = reinterpret_cast<T*>(rm_smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int n = blockIdx.y, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int ty0 = ty * C::TH, tx0 = tx * C::TW;
  const size_t img = (size_t)H * W;
  uint32_t* mimg = mask ? mask + n * img : nullptr;
  rm_stage<T, CI, C::CS, C::SW, C::NPIX, EP == RM_EP_BWD || EP == RM_EP_MSTORE, 256>(tile, in + n * img * CI, mimg, H, W, ty0 - C::P, tx0 - C::P, tid);
  __syncthreads();

  f32x16 acc[C::NRT][C::RPW];
#pragma unroll
  for (int t = 0; t < C::NRT; ++t) {
    f32x16 c0 = zero16();
    if constexpr (EP == RM_EP_BLOCK) {
#pragma unroll
      for (int i = 0; i < 16; ++i) c0[i] = bias[(i & 3) + 8 * (i >> 2) + 4 * hh];
    }
#pragma unroll
    for (int q = 0; q < C::RPW; ++q) acc[t][q] = c0;
  }
  const int row0 = wave * C::RPW;
#pragma unroll 2
  for (int s = 0; s < C::KS; ++s) {
    const int kk = 16 * s + 8 * hh, tap = kk / CI, ci0 = kk - tap * CI;
    const int dy = tap / K, dx = tap - dy * K;
    const bool live = tap < K * K;
    FragT a[C::NRT];
#pragma unroll
    for (int t = 0; t < C::NRT; ++t) a[t] = load_wfrag<T>(wp, t * C::KS + s, lane);
#pragma unroll
    for (int q = 0; q < C::RPW; ++q) {
      FragT b;
      if (live) {
        b = lds_chunk<T>(tile, ((row0 + q + dy) * C::SW + r + dx) * C::CS + ci0);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] = (T)0.f;
      }
#pragma unroll
      for (int t = 0; t < C::NRT; ++t) acc[t][q] = mma16<T>(a[t], b, acc[t][q]);
    }
  }

  const int X = tx0 + r;
#pragma unroll
  for (int q = 0; q < C::RPW; ++q) {
    const int Y = ty0 + row0 + q;
    const bool inside = Y < H && X < W;
    const size_t pix = n * img + (size_t)Y * W + X;
    uint32_t mbits = 0;
#pragma unroll
    for (int t = 0; t < C::NRT; ++t) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c0 = 32 * t + 8 * g + 4 * hh;                    // regs 4g..4g+3 = channels c0..c0+3 of pixel r
        if constexpr (EP == RM_EP_SHUF) {
          if (inside) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int ch = c0 + i;
              if (ch < COUT) {
                const int c = ch / (R * R), rem = ch - c * R * R, si = rem / R, sj = rem - si * R;
                float* o = hr + (((size_t)n * 3 + c) * H * R + (size_t)Y * R + si) * ((size_t)W * R) + (size_t)X * R + sj;
                *o += acc[t][q][4 * g + i];
              }
            }
          }
        } else if (c0 < COUT) {
          float v[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = acc[t][q][4 * g + i];
          if constexpr (EP == RM_EP_BLOCK) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              mbits |= (v[i] > 0.f ? 1u : 0u) << (c0 + i);
              v[i] = fmaxf(v[i], 0.f);
            }
          }
          if (inside) {
            if constexpr (EP == RM_EP_BLOCK || EP == RM_EP_BWD) {
              const HalfT x4 = *reinterpret_cast<const HalfT*>(res + pix * COUT + c0);
#pragma unroll
              for (int i = 0; i < 4; ++i) v[i] += (float)x4[i];
            }
            HalfT o4;
            T e0, e1, e2, e3;
            cvt_pair<T>(e0, e1, v[0], v[1]);
            cvt_pair<T>(e2, e3, v[2], v[3]);
            o4[0] = e0; o4[1] = e1; o4[2] = e2; o4[3] = e3;
            *reinterpret_cast<HalfT*>(out + pix * COUT + c0) = o4;
          }
        }
      }
    }
    if constexpr (EP == RM_EP_BLOCK) {
      mbits |= __shfl_xor(mbits, 32);
      if (inside && hh == 0) mask[pix] = mbits;
    }
  }
}

// ---- weight gradient -------------------------------------------------------------------------------------------------
template <typename T, int K, int CA, int CB>
struct RmWgradCfg {
  static constexpr int P = K / 2, TW = 16, TH = 16, NPX = TW * TH, KSP = NPX / 16;
  static constexpr int SWB = TW + 2 * P, SHB = TH + 2 * P, NPB = SWB * SHB;
  static constexpr int NRT = (CA + 31) / 32, CAS = 32 * NRT, CBS = 32;          // LDS pixel strides (zero-padded channels)
  static constexpr int NTAP = K * K + 1;                                        // K*K taps + the bias tile
  static constexpr int NTL = NRT * NTAP, NW = 8, TPW = 4, TPG = NW * TPW, NG = (NTL + TPG - 1) / TPG;
  static constexpr int LDS_BYTES = (NPX * CAS + NPB * CBS) * (int)sizeof(T);
  static constexpr int SLAB = NTL * 1024;                                       // floats per workgroup slab
};

// NHWC image (CH real channels) -> LDS rows of CS >= CH channels, zero-padded; MASK as in rm_stage
template <typename T, int CH, int CS, int RW, int NPIX, bool MASK, int NTHREADS>
SR_DEV void rm_stage_pad(T* dst, const T* __restrict__ src, const uint32_t* __restrict__ mask, int H, int W, int y0, int x0,
                         int tid) {
  typedef typename FragOf<T>::type FragT;
  constexpr int NC = CS / 8, TOTAL = NPIX * NC;
  for (int idx = tid; idx < TOTAL; idx += NTHREADS) {
    const int p = idx / NC, c = idx - p * NC;
    const int py = p / RW, px = p - py * RW;
    const int Y = y0 + py, X = x0 + px;
    FragT v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (T)0.f;
    if (c * 8 < CH && Y >= 0 && Y < H && X >= 0 && X < W) {
      const size_t pix = (size_t)Y * W + X;
      v = *reinterpret_cast<const FragT*>(src + pix * CH + c * 8);
      if constexpr (MASK) {
        const uint32_t m = mask[pix] >> (c * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (!((m >> j) & 1u)) v[j] = (T)0.f;
      }
    }
    *reinterpret_cast<FragT*>(dst + p * CS + c * 8) = v;
  }
}

// g: NHWC [N,H,W,CA] (masked by `mask` when MASK); xin: NHWC [N,H,W,CB]; partial[NG * gridDim.x][TPG tiles][16][64]:
// tile g * TPG + j of workgroup w at partial + ((g * gridDim.x + w) * TPG + j) * 1024.  Tile (rt, tap) = rt * NTAP + tap.
template <typename T, int K, int CA, int CB, bool MASK>
__global__ void __launch_bounds__(512) rm_wgrad_kernel(const T* __restrict__ g, const uint32_t* __restrict__ mask,
                                                       const T* __restrict__ xin, float* __restrict__ partial, int N, int H,
                                                       int W, int tiles_x, int tiles_per_img) {
  typedef RmWgradCfg<T, K, CA, CB> C;
  typedef typename FragOf<T>::type FragT;
  __shared__ __attribute__((aligned(16))) unsigned char rm_smem[C::LDS_BYTES];
  T* GA = reinterpret_cast<T*>(rm_smem);
  T* XB = GA + C::NPX * C::CAS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = blockIdx.y;
  const size_t img = (size_t)H * W;
  f32x16 acc[C::TPW];
#pragma unroll
  for (int j = 0; j < C::TPW; ++j) acc[j] = zero16();
  FragT ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = (T)1.f;
  const int total = N * tiles_per_img;
  for (int it = blockIdx.x; it < total; it += gridDim.x) {
    const int n = it / tiles_per_img, ti = it - n * tiles_per_img;
    const int ty = ti / tiles_x, tx = ti - ty * tiles_x;
    const int ty0 = ty * C::TH, tx0 = tx * C::TW;
    __syncthreads();                                               // the previous tile's reads are done
    rm_stage_pad<T, CA, C::CAS, C::TW, C::NPX, MASK, 512>(GA, g + n * img * CA, MASK ? mask + n * img : nullptr, H, W, ty0,
                                                          tx0, tid);
    rm_stage_pad<T, CB, C::CBS, C::SWB, C::NPB, false, 512>(XB, xin + n * img * CB, nullptr, H, W, ty0 - C::P, tx0 - C::P,
                                                            tid);
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < C::KSP; ++s) {
#pragma unroll
      for (int j = 0; j < C::TPW; ++j) {
        const int t = grp * C::TPG + j * C::NW + wave;             // wave-uniform
        if (t < C::NTL) {
          const int rt = t / C::NTAP, tap = t - rt * C::NTAP;
          const FragT a = tr_frag<T>(GA, s, lane, [&](int p) { return p * C::CAS + 32 * rt; });
          FragT b;
          if (tap == K * K) {
            b = ones;
          } else {
            const int dy = tap / K, dx = tap - dy * K;
            b = tr_frag<T>(XB, s, lane, [&](int p) {
              const int py = p >> 4, px = p & 15;
              return ((py + dy) * C::SWB + px + dx) * C::CBS;
            });
          }
          acc[j] = mma16<T>(a, b, acc[j]);
        }
      }
    }
  }
  float* slab = partial + ((size_t)grp * gridDim.x + blockIdx.x) * C::TPG * 1024;
#pragma unroll
  for (int j = 0; j < C::TPW; ++j) slab_store_tile(slab, j * C::NW + wave, acc[j], lane);
}

// ---- tail backward helper: HR gradient (NCHW fp32) -> un-shuffled LR image NHWC [N,H,W,CP] in T, zero past 3 R^2 ----
template <typename T, int R, int CP>
__global__ void __launch_bounds__(256) rm_unshuffle_kernel(const float* __restrict__ dout, T* __restrict__ dconv, int N, int H,
                                                           int W) {
  constexpr int CO = 3 * R * R;
  const size_t total = (size_t)N * H * W * CP;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(e % CP);
    const size_t pix = e / CP;
    const int X = (int)(pix % W), Y = (int)((pix / W) % H), n = (int)(pix / ((size_t)H * W));
    float v = 0.f;
    if (ch < CO) {
      const int c = ch / (R * R), rem = ch - c * R * R, si = rem / R, sj = rem - si * R;
      v = dout[(((size_t)n * 3 + c) * H * R + (size_t)Y * R + si) * ((size_t)W * R) + (size_t)X * R + sj];
    }
    dconv[e] = (T)v;
  }
}
