// Per-frame video network (models/single_image_model.py Result_Model), the backward of the training route (gfx950).  The convs'
// backward is result_block.h's family at K = 3, CI = COUT = 32 (sr_abi.hip strings the launches together); new here:
//   fn_up_bwd_kernel   the backward of ConvTranspose2d(C, 3, 5, stride 4) + the fixed two-tap resize: mv_recon_bwd_kernel's scheme
//                      without its fusion layer, 32 channels wide.  Workgroups walk the 8 x 16 LR tiles of all frames:
//                        dD[d] = (1 - l_d) g[d] + l_{d-1} g[d-1] in both directions (a gather of at most four output gradients, l
//                        as ATen computes it: mv_lambda) -> the tile's (4 TH + 1) x (4 TW + 1) x 3 dD values, fp32 in LDS;
//                        df = W dE (dE = the 75 dD values an LR pixel touches, converted to the hot dtype as the MFMA's B operand),
//                        stored NHWC in the hot dtype;  dW_up = f dE^T and db_up = sum g, accumulated across tiles in registers;
//                      ONE fp32 slab per workgroup: dW_up [32][80] (row = channel, column r = 25 o + 5 ky + kx) | db_up [3] | pad.
//   fn_up_bwd_sized_kernel  the same behind a resize to any output size: only the first stage differs, dD gathered over the adjoint
//                      ranges of packing.resize_axis' tables (fn_up_bwd_gather_sized).  <T, LOSS> as fn_up_bwd_kernel below.
//   fn_add_kernel      de = dx_0 + df, the gradient at e (e feeds block 0 and the body's residual).
//   fn_reduce_kernel   every parameter gradient of the network from its workgroup slabs, summed in workgroup order, written in the
//                      reference's tensor shapes: segment j < 2 nb + 1: conv j (rm_wgrad_kernel's slab), 2 nb + 1: the upsampler,
//                      2 nb + 2: the encoder (sr_head_wgrad_kernel's slab).  One launch, grid.y = segment.
// Backward blob (packing.fn_bwd_tables), elements of T: conv j at j * 18 * 512 = rm_conv_kernel's 18 fragments of W^T with both
// taps flipped; the upsampler at (2 nb + 1) * 18 * 512 = 2 x 3 fragments of the 16 x 16 x 32 MFMA, A[c][r] = W[c][r], r padded to 96.
// fn_up_bwd_kernel<T, LOSS> with LOSS = 1 (L1) / 2 (Charbonnier, eps 1e-12) is the same kernel with the trainers' loss folded into
// its first stage (sr_fn_net_bwd_loss): `gout` is then the network's OUTPUT sr and `li.hr` the target with the same image stride, and
// every output gradient the stage would have loaded is formed in registers, wdsr_ends.h's loss_grad<LOSS>(sr, hr, gscale), fp32.  The
// db_up loop visits exactly the tile's own 4 TH x 4 TW outputs -- every HR pixel belongs to one tile's core -- so the loss terms are
// collected there, once per pixel; the dD gather's reads (core and halo) form the same gradient and add nothing to the loss.  The
// per-thread sums go through the dd tile after the walk (fn_sum8, fixed order) into loss_part[workgroup].  Same LDS as LOSS = 0.
// fn_up_bwd_sized_kernel<T, LOSS> folds the same way at any output size: the loss terms are collected in the gather's gsum loop, which
// visits exactly the outputs whose (i0_y, i0_x) the tile owns by the forward's rule, each once; at a downscale most tiles own no
// output, and a workgroup that walked only such tiles writes loss_part = 0.  No atomics anywhere.
#pragma once
#include "mv_recon.h"
#include "wdsr_ends.h"
#include "frame_net.h"
#include "result_block.h"

struct FnBwdCfg {
  static constexpr int NT = 256, NW = 4, TH = FnCfg::UTH, TW = FnCfg::UTW, NPC = TH * TW, RS = FnCfg::RS;
  static constexpr int DH = FnCfg::DH, DW = FnCfg::DW, ND = FnCfg::ND, EB = FnCfg::EB, KSB = 3, MB = 2;
  static constexpr int CONV_ELEMS = FnCfg::KS * 512, UP_ELEMS = MB * KSB * 512;
  static constexpr int SLAB_W = 0, SLAB_B = 32 * 80, SLAB = SLAB_B + 16;       // one workgroup's upsampler slab
  static constexpr int CONV_SLAB = 32 * 1024, HEAD_SLAB = 3 * 1024;            // rm_wgrad_kernel's (K = 3, one tile group), sr_head_wgrad's
};

// sum of n floats `stride` apart in a FIXED order: eight interleaved running sums, then a three-level tree.  Shorter chains than
// one running sum (the rounding error of a long fp32 chain grows with its length), and eight independent loads in flight.
SR_DEV float fn_sum8(const float* __restrict__ p, int n, size_t stride) {
  float t[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int k = 0;
  for (; k + 8 <= n; k += 8)
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] += p[(size_t)(k + j) * stride];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (k + j < n) t[j] += p[(size_t)(k + j) * stride];
  return ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
}

// The first stage of fn_up_bwd_sized_kernel for one tile: g is one image's (3, OH, OW) output gradient (LOSS != 0: the network's
// output sr, hr the target at the same offsets, every g[..] below is then loss_grad<LOSS>(sr, hr, gscale), fp32), (r0, c0) the tile's first D
// row and column, bottom / right: the tile ends the image.  The resize's adjoint as a GATHER over rz's ranges (FnResize):
//   dD[a] = sum over outputs r with i0 == a of (1 - lam[r]) g[r]  (weight 1 at a == 4H: there i1 == i0, both taps read row a)
//         + sum over outputs r with i0 == a - 1 of lam[r] g[r]      (their second tap, i1 == a)
// in both directions, ranges ascending, rows outside columns inside, fp32.  D cells no output reads (and cells past the image) get 0.
// gsum += g over the outputs whose (i0_y, i0_x) this tile OWNS, the forward's rule (fn_up_sized_kernel): every output once; lsum +=
// their loss terms there and only there (the dD loops form the same gradients again and add nothing to the loss).
template <int LOSS>
SR_DEV void fn_up_bwd_gather_sized(const float* __restrict__ g, [[maybe_unused]] const float* __restrict__ hq,
                                   [[maybe_unused]] float gscale, const FnResize& rz, int H4, int W4, int r0, int c0, bool bottom,
                                   bool right, float* __restrict__ dd, float (&gsum)[3], [[maybe_unused]] float& lsum) {
  typedef FnBwdCfg C;
  const int tid = threadIdx.x;
  const int* const lo_y = rz.ty + rz.OH;
  const int* const hi_y = lo_y + H4 + 1;
  const int* const lo_x = rz.tx + rz.OW;
  const int* const hi_x = lo_x + W4 + 1;
  const size_t plane = (size_t)rz.OH * rz.OW;
  const int r1 = bottom ? H4 : r0 + 4 * C::TH - 1, c1 = right ? W4 : c0 + 4 * C::TW - 1;
  [[maybe_unused]] auto grad_at = [&](size_t off, float& term) -> float {
    if constexpr (LOSS == 0) {
      return g[off];
    } else {
      return loss_grad<LOSS>(g[off], hq[off], gscale, term);
    }
  };
  const int oy0 = lo_y[r0], ny = hi_y[r1] - oy0 + 1, ox0 = lo_x[c0], nx = hi_x[c1] - ox0 + 1;      // >= 0 each
  for (int idx = tid; idx < ny * nx; idx += C::NT) {
    const int ry = idx / nx;
    const size_t off = (size_t)(oy0 + ry) * rz.OW + ox0 + (idx - ry * nx);
    if constexpr (LOSS == 0) {
      gsum[0] += g[off];
      gsum[1] += g[plane + off];
      gsum[2] += g[2 * plane + off];
    } else {
#pragma unroll
      for (int o = 0; o < 3; ++o) {
        float term = 0.f;
        gsum[o] += grad_at(o * plane + off, term);
        lsum += term;
      }
    }
  }
  for (int idx = tid; idx < C::ND; idx += C::NT) {
    const int o = idx / (C::DH * C::DW), rem = idx - o * (C::DH * C::DW);
    const int dy = rem / C::DW, dx = rem - dy * C::DW;
    const int a = r0 + dy, e = c0 + dx;
    float v = 0.f;
    if (a <= H4 && e <= W4) {
      [[maybe_unused]] const float* const go = g + o * plane;
#pragma unroll
      for (int ky = 0; ky < 2; ++ky) {
        const int ia = a - ky;
        if (ia < 0) continue;
        for (int r = lo_y[ia]; r <= hi_y[ia]; ++r) {
          const float wy = ky ? rz.ly[r] : a == H4 ? 1.f : 1.f - rz.ly[r];
          [[maybe_unused]] const float* const grow = go + (size_t)r * rz.OW;
          float row = 0.f;
#pragma unroll
          for (int kx = 0; kx < 2; ++kx) {
            const int ie = e - kx;
            if (ie < 0) continue;
            for (int c = lo_x[ie]; c <= hi_x[ie]; ++c) {
              const float wx = kx ? rz.lx[c] : e == W4 ? 1.f : 1.f - rz.lx[c];
              if constexpr (LOSS == 0) {
                row += wx * grow[c];
              } else {
                float term;
                row += wx * grad_at(o * plane + (size_t)r * rz.OW + c, term);
              }
            }
          }
          v += wy * row;
        }
      }
    }
    dd[idx] = v;
  }
}

// f, df: [frame][H][W][32]; gout: frame n at gout + n * g_is, NCHW fp32 (3, 4H, 4W); wlb: the upsampler's backward fragments;
// slab of workgroup w at parts + w * SLAB; items = frames x tiles.  LOSS != 0: gout = sr, li.hr = the target (image n at + n * g_is
// both), loss_part[workgroup] = this workgroup's share of the loss sum
// SIZED: gout (and li.hr) is (3, OH, OW) and the first stage reads rz's tables, see fn_up_bwd_sized_kernel
template <typename T, int LOSS, bool SIZED>
SR_DEV void fn_up_bwd_body(const T* __restrict__ f, const float* __restrict__ gout, long g_is, const T* __restrict__ wlb,
                           T* __restrict__ df, float* __restrict__ parts, int N, int H, int W, int tiles_x, int tiles, LossIn li,
                           float* __restrict__ loss_part, const FnResize& rz) {
  typedef FnBwdCfg C;
  typedef typename FragOf<T>::type FragT;
  typedef typename FragOf<T>::half_type HalfT;
  __shared__ __attribute__((aligned(32))) float dd[C::ND + 5];               // the dD tile; afterwards the db_up reduction
  __shared__ __attribute__((aligned(32))) T fs[C::NPC * C::RS];
  __shared__ int koff[96];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, q = lane >> 4;
  if (tid < 96) koff[tid] = tid < 75 ? ((tid / 25) * C::DH + (tid % 25) / 5) * C::DW + tid % 5 : -1;
  const int H4 = 4 * H, W4 = 4 * W;
  [[maybe_unused]] const float sy = (float)(H4 + 1) / (float)H4, sx = (float)(W4 + 1) / (float)W4;
  f32x4 accl[C::EB];
#pragma unroll
  for (int e = 0; e < C::EB; ++e) accl[e] = f32x4{0.f, 0.f, 0.f, 0.f};
  float gsum[3] = {0.f, 0.f, 0.f};
  [[maybe_unused]] float lsum = 0.f;
  const int items = N * tiles;
#pragma unroll 1
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int tile = item % tiles, n = item / tiles;
    const int ty0 = (tile / tiles_x) * C::TH, tx0 = (tile % tiles_x) * C::TW;
    const size_t img = (size_t)n * H * W;
    const float* const g = gout + (size_t)n * g_is;
    [[maybe_unused]] const float* const hq = LOSS ? li.hr + (size_t)n * g_is : nullptr;
    // the output gradient at element `off` of this image: loaded, or formed from sr and hr (term: the element's loss term)
    [[maybe_unused]] auto grad_at = [&](size_t off, float& term) -> float {
      if constexpr (LOSS == 0) {
        return g[off];
      } else {
        return loss_grad<LOSS>(g[off], hq[off], li.gscale, term);
      }
    };
    __syncthreads();                                       // the previous tile's readers are done (and koff is written)
    for (int idx = tid; idx < C::NPC * 4; idx += C::NT) {
      const int p = idx >> 2, cc = idx & 3;
      const int Y = ty0 + p / C::TW, X = tx0 + p % C::TW;
      FragT v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (T)0.f;
      if (Y < H && X < W) v = *reinterpret_cast<const FragT*>(f + (img + (size_t)Y * W + X) * 32 + cc * 8);
      *reinterpret_cast<FragT*>(fs + p * C::RS + cc * 8) = v;
    }
    if constexpr (SIZED) {
      fn_up_bwd_gather_sized<LOSS>(g, hq, li.gscale, rz, H4, W4, 4 * ty0, 4 * tx0, ty0 + C::TH >= H, tx0 + C::TW >= W, dd, gsum, lsum);
    } else {
      // db_up = sum of dD = sum of the output gradient (the blend's weights sum to one): this tile's own 4 TH x 4 TW outputs
      for (int idx = tid; idx < 3 * 16 * C::NPC; idx += C::NT) {
        const int o = idx / (16 * C::NPC), rem = idx - o * (16 * C::NPC);
        const int Y = 4 * ty0 + rem / (4 * C::TW), X = 4 * tx0 + rem % (4 * C::TW);
        float v = 0.f;
        if (Y < H4 && X < W4) {
          [[maybe_unused]] float term = 0.f;
          v = grad_at(((size_t)o * H4 + Y) * W4 + X, term);
          if constexpr (LOSS != 0) lsum += term;
        }
        if (o == 0) gsum[0] += v; else if (o == 1) gsum[1] += v; else gsum[2] += v;
      }
      // dD[a][e] = sum over the (at most) four outputs that read it
      for (int idx = tid; idx < C::ND; idx += C::NT) {
        const int o = idx / (C::DH * C::DW), rem = idx - o * (C::DH * C::DW);
        const int dy = rem / C::DW, dx = rem - dy * C::DW;
        const int a = 4 * ty0 + dy, e = 4 * tx0 + dx;
        const size_t go = (size_t)o * H4 * W4;
        [[maybe_unused]] float term;
        const float wy0 = a < H4 ? 1.f - mv_lambda(a, sy) : 0.f, wy1 = (a >= 1 && a <= H4) ? mv_lambda(a - 1, sy) : 0.f;
        const float wx0 = e < W4 ? 1.f - mv_lambda(e, sx) : 0.f, wx1 = (e >= 1 && e <= W4) ? mv_lambda(e - 1, sx) : 0.f;
        float v = 0.f;
        if (a < H4) {
          if (e < W4) v += wy0 * wx0 * grad_at(go + (size_t)a * W4 + e, term);
          if (e >= 1 && e <= W4) v += wy0 * wx1 * grad_at(go + (size_t)a * W4 + e - 1, term);
        }
        if (a >= 1 && a <= H4) {
          if (e < W4) v += wy1 * wx0 * grad_at(go + (size_t)(a - 1) * W4 + e, term);
          if (e >= 1 && e <= W4) v += wy1 * wx1 * grad_at(go + (size_t)(a - 1) * W4 + e - 1, term);
        }
        dd[idx] = v;
      }
    }
    __syncthreads();
    // df = W dE, 16 pixels at a time
#pragma unroll 1
    for (int gq = wave; gq < C::NPC / 16; gq += C::NW) {
      const int p = gq * 16 + l16;
      const int ly = p / C::TW, lx = p % C::TW;
      const int Y = ty0 + ly, X = tx0 + lx;
      const int pixoff = 4 * ly * C::DW + 4 * lx;
      f32x4 du[C::MB];
#pragma unroll
      for (int m = 0; m < C::MB; ++m) du[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < C::KSB; ++s) {
        FragT b;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int ko = koff[32 * s + 8 * q + j];
          b[j] = (T)(ko >= 0 ? dd[ko + pixoff] : 0.f);
        }
#pragma unroll
        for (int m = 0; m < C::MB; ++m) du[m] = vr_mma32<T>(load_wfrag<T>(wlb, m * C::KSB + s, lane), b, du[m]);
      }
      if (Y < H && X < W) {
#pragma unroll
        for (int m = 0; m < C::MB; ++m) {
          HalfT v;
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = (T)du[m][i];
          *reinterpret_cast<HalfT*>(df + (img + (size_t)Y * W + X) * 32 + 16 * m + 4 * q) = v;
        }
      }
    }
    // dW_up: wave m owns rows 16 m .. 16 m + 15 (channels of f); the contraction runs over the tile's pixels
    if (wave < C::MB) {
      const int row = 16 * wave + l16;
#pragma unroll 1
      for (int s = 0; s < C::NPC / 32; ++s) {
        FragT au;
        int po[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int p = 32 * s + 8 * q + j;
          au[j] = fs[p * C::RS + row];
          po[j] = 4 * (p / C::TW) * C::DW + 4 * (p % C::TW);
        }
#pragma unroll
        for (int eb = 0; eb < C::EB; ++eb) {
          const int ko = koff[16 * eb + l16];
          FragT b;
#pragma unroll
          for (int j = 0; j < 8; ++j) b[j] = (T)(ko >= 0 ? dd[ko + po[j]] : 0.f);
          accl[eb] = vr_mma32<T>(au, b, accl[eb]);
        }
      }
    }
  }
  float* const slab = parts + (size_t)blockIdx.x * C::SLAB;
  if (wave < C::MB) {
#pragma unroll
    for (int eb = 0; eb < C::EB; ++eb)
#pragma unroll
      for (int i = 0; i < 4; ++i) slab[C::SLAB_W + (16 * wave + 4 * q + i) * 80 + 16 * eb + l16] = accl[eb][i];
  }
  __syncthreads();
#pragma unroll
  for (int o = 0; o < 3; ++o) dd[o * C::NT + tid] = gsum[o];
  if constexpr (LOSS != 0) dd[3 * C::NT + tid] = lsum;
  __syncthreads();
  if (tid < 3) slab[C::SLAB_B + tid] = fn_sum8(dd + tid * C::NT, C::NT, 1);
  if constexpr (LOSS != 0) {
    if (tid == 64) loss_part[blockIdx.x] = fn_sum8(dd + 3 * C::NT, C::NT, 1);
  }
}

template <typename T, int LOSS = 0>
__global__ __launch_bounds__(256) void fn_up_bwd_kernel(const T* __restrict__ f, const float* __restrict__ gout, long g_is,
                                                        const T* __restrict__ wlb, T* __restrict__ df, float* __restrict__ parts,
                                                        int N, int H, int W, int tiles_x, int tiles, LossIn li = LossIn{nullptr, 0.f},
                                                        float* __restrict__ loss_part = nullptr) {
  fn_up_bwd_body<T, LOSS, false>(f, gout, g_is, wlb, df, parts, N, H, W, tiles_x, tiles, li, loss_part, FnResize{});
}

// fn_up_bwd_kernel<T, LOSS> behind a resize to any (OH, OW): gout (3, OH, OW), the first stage is fn_up_bwd_gather_sized; df, the
// dW_up slab and the reduction are unchanged.  No atomics: two equal calls give the same bits.
template <typename T, int LOSS = 0>
__global__ __launch_bounds__(256) void fn_up_bwd_sized_kernel(const T* __restrict__ f, const float* __restrict__ gout, long g_is,
                                                              const T* __restrict__ wlb, T* __restrict__ df, float* __restrict__ parts,
                                                              int N, int H, int W, int tiles_x, int tiles, FnResize rz,
                                                              LossIn li = LossIn{nullptr, 0.f}, float* __restrict__ loss_part = nullptr) {
  fn_up_bwd_body<T, LOSS, true>(f, gout, g_is, wlb, df, parts, N, H, W, tiles_x, tiles, li, loss_part, rz);
}

// y = a + b over n_vec groups of 4 elements (fp32 sum, one rounding)
template <typename T>
__global__ __launch_bounds__(256) void fn_add_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ y, size_t n_vec) {
  typedef typename FragOf<T>::half_type HalfT;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec; i += (size_t)gridDim.x * blockDim.x) {
    const HalfT u = reinterpret_cast<const HalfT*>(a)[i], v = reinterpret_cast<const HalfT*>(b)[i];
    HalfT o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (T)((float)u[j] + (float)v[j]);
    reinterpret_cast<HalfT*>(y)[i] = o;
  }
}

// element (row, col) of 32 x 32 accumulator tile `tile` in a [tile][reg 16][lane 64] slab (packing._acc_pos)
SR_DEV int fn_acc_pos(int tile, int row, int col) {
  return (tile * 16 + (row & 3) + 4 * (row >> 3)) * 64 + col + 32 * ((row >> 2) & 1);
}

// parts: conv slabs [2 nb + 1][wgs][CONV_SLAB] | upsampler [wgs][SLAB], the first up_wgs written | encoder [wgs][HEAD_SLAB].  grads: conv j's dW (C, C, 3, 3)
// | db (C) at j (9 C C + C); then the upsampler's dW (C, 3, 5, 5) | db (3); then the encoder's dW (C, 3, 3, 3) | db (C).
// do_*: which stages' segments are reduced (the others' slabs were not written by this call)
__global__ __launch_bounds__(256) void fn_reduce_kernel(const float* __restrict__ parts, float* __restrict__ grads, int C, int nb,
                                                        int wgs, int up_wgs, int do_blocks, int do_last, int do_up, int do_enc) {
  typedef FnBwdCfg B;
  const int seg = blockIdx.y, nconv = 2 * nb + 1, per = 9 * C * C + C;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const float* src;
  float* dst;
  int off, n, stride;
  if (seg < nconv) {
    if (!(seg < nconv - 1 ? do_blocks : do_last) || i >= per) return;
    src = parts + (size_t)seg * wgs * B::CONV_SLAB;
    dst = grads + (size_t)seg * per;
    n = wgs, stride = B::CONV_SLAB;
    if (i < 9 * C * C) {
      const int co = i / (9 * C), ci = i / 9 % C, tap = i % 9;
      off = fn_acc_pos(tap, co, ci);
    } else {
      off = fn_acc_pos(9, i - 9 * C * C, 0);
    }
  } else if (seg == nconv) {
    if (!do_up || i >= 75 * C + 3) return;
    src = parts + (size_t)nconv * wgs * B::CONV_SLAB;
    dst = grads + (size_t)nconv * per;
    n = up_wgs, stride = B::SLAB;
    off = i < 75 * C ? B::SLAB_W + (i / 75) * 80 + i % 75 : B::SLAB_B + i - 75 * C;
  } else {
    if (!do_enc || i >= 28 * C) return;
    src = parts + (size_t)nconv * wgs * B::CONV_SLAB + (size_t)wgs * B::SLAB;
    dst = grads + (size_t)nconv * per + 75 * C + 3;
    n = wgs, stride = B::HEAD_SLAB;
    if (i < 27 * C) {
      const int co = i / 27, ci = i / 9 % 3, ky = i / 3 % 3, kx = i % 3;
      off = fn_acc_pos(ky, co, 4 * kx + ci);
    } else {
      off = fn_acc_pos(1, i - 27 * C, 7);                 // the ones channel at the centre tap
    }
  }
  dst[i] = fn_sum8(src + off, n, stride);
}
