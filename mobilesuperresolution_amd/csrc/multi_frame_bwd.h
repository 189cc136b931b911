// Multi-frame video network (models/naive_multi_model_easy.py Naive_model), the backward of the training route (gfx950).  The convs'
// backward is result_block.h's family at K = 3 (sr_abi.hip strings the launches together: rm_unshuffle, rm_conv with EP_STORE / EP_BWD
// / EP_MSTORE, rm_wgrad, sr_head_wgrad); new here:
//   mf_warp_bwd_kernel  the gradient at e, all of its three sources in one pass.  Frame n = b NF + i:
//                         de_n = de_direct_n + (i == 0 ? dwarp_n : 0) + (i < NF - 1 ? sum_o w_tap(o) dwarp_{n+1}[o] : 0)
//                       de_direct = dy + conv1_e^T(dt * mask) (e feeds block 0's e group and its residual), dwarp = conv1_warp^T(dt *
//                       mask); frame 0 of a clip warps nothing, its warp operand IS e_0; frame n + 1's warp operand sampled e_n.  The
//                       last sum is flow_warp's backward in GATHER form (c3_warp_bwd_kernel's scheme at 32 NHWC channels): one thread
//                       per source pixel, 16 x 16 per workgroup, walks the output pixels o of frame n + 1 with |o - s| <= RW, RW =
//                       ceil(max |flow|) + 1 read from a device scalar, clipped to the image; the candidates' taps (warp_pos /
//                       warp_taps, the forward's arithmetic) sit in LDS up to RW = 7 and are recomputed beyond.  Row-major window
//                       order, fp32, one rounding to T.  A clip's last frame reads no next frame, frame 0 sends nothing back.
//   mf_dd_loss_kernel   the tail backward's first stage with a loss source (sr_mf_net_bwd_loss): dD formed from sr and hr, see below.
//   mf_reduce_kernel    every parameter gradient from its workgroup slabs, summed in workgroup order (fn_sum8), written in the
//                       reference's shapes; block 0's conv1 (C, 2C + 2, 3, 3) is assembled from its three groups' slabs in
//                       cat(flow, warp, e) order.  One launch, grid.y = segment.
// Backward blob (packing.mf_bwd_tables), elements of T, each conv rm_conv_kernel's fragments of W^T with both taps flipped: block 0 =
// [e group 18][warp group 18][conv2 18]; blocks 1.. = [conv1 18][conv2 18]; decode = 27 fragments (K = 9 x 48 -> 32 rows).
// No atomics anywhere.
#pragma once
#include <climits>
#include "multi_frame.h"
#include "frame_net_bwd.h"

struct MfBwdCfg {
  static constexpr int CONV_ELEMS = FnCfg::KS * 512, DEC_ELEMS = 27 * 512;
  static constexpr int CONV_SLAB = FnBwdCfg::CONV_SLAB, HEAD_SLAB = FnBwdCfg::HEAD_SLAB;
  static constexpr int TS = 16, RW_LDS = 7, CW = TS + 2 * RW_LDS, NCAND = CW * CW;
  // element offset of block i's conv1 (block 0: its e group; the warp group and conv2 follow) and of the decode conv
  static constexpr size_t block_off(int i) { return i == 0 ? 0 : (size_t)(3 + 2 * (i - 1)) * CONV_ELEMS; }
  static constexpr size_t dec_off(int nb) { return (size_t)(2 * nb + 1) * CONV_ELEMS; }
};

// taps of output pixel (oy, ox) of the frame whose flow plane pair starts at fl
SR_DEV WarpTaps mf_taps_of(const float* __restrict__ fl, size_t plane, int oy, int ox, int H, int W) {
  const size_t pix = (size_t)oy * W + ox;
  return warp_taps(warp_pos((float)ox + fl[pix], W), warp_pos((float)oy + fl[plane + pix], H), H, W);
}

// The tail backward's first stage with a loss source (sr_mf_net_bwd_loss): what rm_unshuffle_kernel<T, 4, 48> reads from g is formed
// here from the network's output sr and the target hr, wdsr_ends.h's loss_grad<LOSS> (1: L1, 2: Charbonnier, eps 1e-12) in fp32, and
// stored as the same dD image [frame][H][W][48] (channel 16 c + 4 i + j = HR pixel (4 Y + i, 4 X + j) of colour c), one rounding to T.
// Workgroups walk the 8 x 32 LR tiles of all frames, one thread per LR pixel: its 48 HR values are twelve 16-byte rows of sr and of hr
// (a wave reads two 512-byte runs per row) and one contiguous 48-element store.  The un-shuffle has no halo: every HR pixel is read by
// exactly one thread, which adds its loss term (|d| resp. sqrt(d^2 + eps)) to its running sum in (item, c, i, j) order; the 256 sums
// are reduced in a fixed order (fn_sum8) into loss_part[workgroup].  sr, hr: contiguous fp32 [frames][3][4H][4W].
struct MfLossCfg {
  static constexpr int NT = 256, TH = 8, TW = 32;
};
template <typename T, int LOSS>
__global__ __launch_bounds__(256) void mf_dd_loss_kernel(const float* __restrict__ sr, const float* __restrict__ hr, float gscale,
                                                         T* __restrict__ dD, float* __restrict__ loss_part, int NF, int H, int W,
                                                         int tiles_x, int tiles) {
  typedef MfLossCfg C;
  typedef typename FragOf<T>::half_type HalfT;
  __shared__ float red[C::NT];
  const int tid = threadIdx.x, ly = tid / C::TW, lx = tid % C::TW;
  const size_t W4 = 4 * (size_t)W, plane = 4 * (size_t)H * W4;
  float lsum = 0.f;
  const int items = NF * tiles;
#pragma unroll 1
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int tile = item % tiles, n = item / tiles;
    const int Y = (tile / tiles_x) * C::TH + ly, X = (tile % tiles_x) * C::TW + lx;
    if (Y >= H || X >= W) continue;
    const size_t base = (size_t)n * 3 * plane + 4 * (size_t)Y * W4 + 4 * (size_t)X;
    T* const d = dD + (((size_t)n * H + Y) * W + X) * 48;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const size_t off = base + c * plane + i * W4;
        const f32x4 q = *reinterpret_cast<const f32x4*>(sr + off), h = *reinterpret_cast<const f32x4*>(hr + off);
        HalfT v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float term;
          v[j] = (T)loss_grad<LOSS>(q[j], h[j], gscale, term);
          lsum += term;
        }
        *reinterpret_cast<HalfT*>(d + 16 * c + 4 * i) = v;
      }
    }
  }
  red[tid] = lsum;
  __syncthreads();
  if (tid == 0) loss_part[blockIdx.x] = fn_sum8(red, C::NT, 1);
}

// direct, dwarp, de: [frame][H][W][32]; flows: fp32 (B, NF - 1, 2, H, W); flow_bound: device scalar >= max |flow| (unused when NF == 1)
template <typename T>
__global__ __launch_bounds__(256) void mf_warp_bwd_kernel(const T* __restrict__ direct, const T* __restrict__ dwarp,
                                                          const float* __restrict__ flows, const float* __restrict__ flow_bound,
                                                          T* __restrict__ de, int H, int W, int tiles_x, int NF) {
  typedef typename FragOf<T>::type FragT;
  typedef MfBwdCfg B;
  __shared__ int2 tap_xy[B::NCAND];                  // (x0, y0) of every candidate output pixel; x0 = INT_MIN: outside the image
  __shared__ float2 tap_w[B::NCAND];                 // (wx, wy)
  const int n = blockIdx.y, tile = blockIdx.x;
  const int clip = n / NF, fi = n - clip * NF;
  const bool has_next = fi + 1 < NF;                 // block-uniform
  const int ty0 = (tile / tiles_x) * B::TS, tx0 = (tile % tiles_x) * B::TS;
  const int sy = ty0 + (int)threadIdx.x / B::TS, sx = tx0 + (int)threadIdx.x % B::TS;
  const size_t plane = (size_t)H * W;
  const float* const fl = has_next ? flows + ((size_t)clip * (NF - 1) + fi) * 2 * plane : nullptr;   // frame n + 1's flow
  int rw = 0;
  if (has_next) {
    const float b = *flow_bound;
    rw = (b < 0.f ? 0 : (b > 1e6f ? 1000000 : (int)ceilf(b))) + 1;
  }
  const bool in_lds = rw <= B::RW_LDS;
  const int cw = B::TS + 2 * rw;
  if (has_next && in_lds) {
    for (int i = threadIdx.x; i < cw * cw; i += 256) {
      const int oy = ty0 - rw + i / cw, ox = tx0 - rw + i % cw;
      int2 xy = {INT_MIN, 0};
      float2 wq = {0.f, 0.f};
      if (oy >= 0 && oy < H && ox >= 0 && ox < W) {
        const WarpTaps t = mf_taps_of(fl, plane, oy, ox, H, W);
        xy.x = t.x0; xy.y = t.y0; wq.x = t.wx; wq.y = t.wy;
      }
      tap_xy[i] = xy;
      tap_w[i] = wq;
    }
    __syncthreads();
  }
  if (sy >= H || sx >= W) return;
  const size_t p = (size_t)n * plane + (size_t)sy * W + sx;
  float acc[32], sum[32];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const FragT d = *reinterpret_cast<const FragT*>(direct + p * 32 + c * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) { acc[c * 8 + j] = (float)d[j]; sum[c * 8 + j] = 0.f; }
  }
  if (fi == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const FragT d = *reinterpret_cast<const FragT*>(dwarp + p * 32 + c * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[c * 8 + j] += (float)d[j];
    }
  }
  if (has_next) {
    const T* const gi = dwarp + (size_t)(n + 1) * plane * 32;
    const int y_lo = sy - rw < 0 ? 0 : sy - rw, y_hi = sy + rw >= H ? H - 1 : sy + rw;
    const int x_lo = sx - rw < 0 ? 0 : sx - rw, x_hi = sx + rw >= W ? W - 1 : sx + rw;
    for (int oy = y_lo; oy <= y_hi; ++oy)
      for (int ox = x_lo; ox <= x_hi; ++ox) {
        int x0, y0;
        float wx, wy;
        if (in_lds) {
          const int i = (oy - (ty0 - rw)) * cw + ox - (tx0 - rw);
          x0 = tap_xy[i].x; y0 = tap_xy[i].y; wx = tap_w[i].x; wy = tap_w[i].y;
        } else {
          const WarpTaps t = mf_taps_of(fl, plane, oy, ox, H, W);
          x0 = t.x0; y0 = t.y0; wx = t.wx; wy = t.wy;
        }
        // long: x0 may be INT_MIN (LDS marker) or the cast of a far position
        const long dy = (long)sy - y0, dx = (long)sx - x0;
        if (dy < 0 || dy > 1 || dx < 0 || dx > 1) continue;
        const float wgt = (dx ? wx : 1.f - wx) * (dy ? wy : 1.f - wy);
        const T* const row = gi + ((size_t)oy * W + ox) * 32;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const FragT q = *reinterpret_cast<const FragT*>(row + c * 8);
#pragma unroll
          for (int j = 0; j < 8; ++j) sum[c * 8 + j] += wgt * (float)q[j];
        }
      }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    FragT o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (T)(acc[c * 8 + j] + sum[c * 8 + j]);
    *reinterpret_cast<FragT*>(de + p * 32 + c * 8) = o;
  }
}

// parts: conv slabs [2 nb + 3][wgs][CONV_SLAB] (slab 2 i: block i's conv1 -- block 0: its e group --, 2 i + 1: its conv2, 2 nb: block 0's
// warp group, 2 nb + 1: its flow group, 2 nb + 2: decode, two row tiles of 10) | encoder [wgs][HEAD_SLAB].  grads: block 0's dW1
// (C, 2C + 2, 3, 3) | db1 (C) | dW2 (C, C, 3, 3) | db2 (C); blocks 1..: the same with dW1 (C, C, 3, 3); decode dW (48, C, 3, 3) | db (48);
// encoder dW (C, 3, 3, 3) | db (C).  Segment 0: block 0's conv1, 1 .. 2 nb - 1: the other block convs, 2 nb: decode, 2 nb + 1: encoder.
// do_*: which stages' segments are reduced (the others' slabs were not written by this call)
__global__ __launch_bounds__(256) void mf_reduce_kernel(const float* __restrict__ parts, float* __restrict__ grads, int C, int nb,
                                                        int wgs, int do_tail, int do_blocks, int do_first, int do_enc) {
  typedef MfBwdCfg B;
  const int seg = blockIdx.y, nconv = 2 * nb, per = 9 * C * C + C, cin0 = 2 * C + 2, first = 9 * C * cin0 + C;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  int slab, off, stride = B::CONV_SLAB;
  float* dst;
  if (seg == 0) {
    if (!do_first || i >= first) return;
    dst = grads;
    if (i < 9 * C * cin0) {
      const int co = i / (9 * cin0), cin = i / 9 % cin0, tap = i % 9;
      const int ci = cin < 2 ? cin : (cin < 2 + C ? cin - 2 : cin - 2 - C);
      slab = cin < 2 ? 2 * nb + 1 : (cin < 2 + C ? 2 * nb : 0);
      off = fn_acc_pos(tap, co, ci);
    } else {
      slab = 0;
      off = fn_acc_pos(9, i - 9 * C * cin0, 0);
    }
  } else if (seg < nconv) {
    if (!(seg == 1 ? do_first : do_blocks) || i >= per) return;
    dst = grads + first + (size_t)(seg - 1) * per;
    slab = seg;
    if (i < 9 * C * C) {
      const int co = i / (9 * C), ci = i / 9 % C, tap = i % 9;
      off = fn_acc_pos(tap, co, ci);
    } else {
      off = fn_acc_pos(9, i - 9 * C * C, 0);
    }
  } else if (seg == nconv) {
    if (!do_tail || i >= 48 * 9 * C + 48) return;
    dst = grads + first + (size_t)(nconv - 1) * per;
    slab = 2 * nb + 2;
    if (i < 48 * 9 * C) {
      const int co = i / (9 * C), ci = i / 9 % C, tap = i % 9;
      off = fn_acc_pos((co >> 5) * 10 + tap, co & 31, ci);
    } else {
      const int co = i - 48 * 9 * C;
      off = fn_acc_pos((co >> 5) * 10 + 9, co & 31, 0);
    }
  } else {
    if (!do_enc || i >= 28 * C) return;
    dst = grads + first + (size_t)(nconv - 1) * per + 48 * 9 * C + 48;
    slab = 2 * nb + 3;
    stride = B::HEAD_SLAB;
    if (i < 27 * C) {
      const int co = i / 27, ci = i / 9 % 3, ky = i / 3 % 3, kx = i % 3;
      off = fn_acc_pos(ky, co, 4 * kx + ci);
    } else {
      off = fn_acc_pos(1, i - 27 * C, 7);                 // the ones channel at the centre tap
    }
  }
  dst[i] = fn_sum8(parts + (size_t)slab * wgs * B::CONV_SLAB + off, wgs, stride);
}
