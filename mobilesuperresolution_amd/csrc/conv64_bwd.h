// 64-feature BasicVSR propagation trunk, the backward of the opt-in training route (gfx950).
// Reference ops differentiated: ConvResidualBlocks / ResidualBlockNoBN (models/basicvsr_arch.py:108-147) and the flow_warp in front of
// the first conv (basicvsr_arch.py:74-76,85-87).
//
// Backward-data needs no kernel of its own: the backward of a 3x3 stride-1 pad-1 conv is that conv with the taps flipped and in / out
// transposed, so c64_conv_kernel (conv64.h) runs it on a backward blob (packing.c64_bwd_tables), with the masked staging DZ forming
// dz = g * act'(A) on the way into LDS and the ADD epilogue carrying the residual.  This file holds the three kernels that have no
// forward counterpart: the weight gradient, the gather-form warp backward (the state's gradient) and, for the opt-in flow_training
// route, the flow gradient of the warp (c64_warp_dflow_kernel).  Rounding points are the 24-wide route's (conv3x3.h):
// ga_i, gt_i, dx0 and dstate are stored in the hot dtype, accumulation is fp32, masks come from the stored t_i / a_0.
#pragma once
#include "conv64.h"

// ---------------------------------------------------------------------------------------------
// weight gradient: dW[co, ci, tap] = sum over pixels p of dz[co, p - tap] x[ci, p], db[co] = sum of dz[co, p].
// Nine waves, wave u owns tap 8 - u (the window offset (u / 3, u % 3) into dz on the tile + 1-pixel halo, x on the core) and holds
// its whole [ci][co] matrix as 32 x 32 accumulator tiles (ci block cb, co block ob): 2 x 2 at CI = 64, 3 x 2 at CI = 80 (x rows are
// staged 96 wide: channels 67..79 and 81..95 zero, channel 80 = 1, whose row of the centre tap is db).  At CI = 64 there is no spare
// channel: the centre-tap wave makes two more tiles from a constant fragment (row 0 = ones).  Both operands are read pixel-major
// from LDS with tr_frag; a k-step is one core row of 16 pixels.  bf16 stages the whole 16 x 16 tile, fp32 two passes of 8 rows
// (LDS: 100 KB either way at CI = 80).  A workgroup walks tiles blockIdx.x, + gridDim.x, ... and writes ONE slab
// [tile][reg 16][lane 64] (packing._acc_pos): tile = u NT + 2 cb + ob with NT = 6 (CI = 80) or 4, then the two db tiles at CI = 64.
// blockIdx.y = layer: all convs of one kind share a launch.  n_dir as c3_wgrad_kernel.
// SUB = 1 (the sub-pixel convs of an upconv + PixelShuffle(2), csrc/vsr_recon_bwd.h): blockIdx.y = q = 2 dy + dx, dA and A are
// [N][2H][2W][64] images and dz of pixel (Y, X) is read at (2Y + dy, 2X + dx): the stride-2 view, no unshuffle pass.
// ---------------------------------------------------------------------------------------------
struct C64Wg {
  static constexpr int NTHREADS = 576, TS = 16, DW = TS + 2;
  template <typename T> static constexpr int rows() { return sizeof(T) == 2 ? 16 : 8; }        // core rows per pass
  static constexpr int xw(int ci) { return ci == 80 ? 96 : 64; }                                 // staged width of an x row
  template <typename T> static constexpr int rsx(int ci) { return xw(ci) + 16 / (int)sizeof(T); }
  template <typename T> static constexpr int rsd() { return 64 + 16 / (int)sizeof(T); }
  static constexpr int nt(int ci) { return ci == 80 ? 6 : 4; }                                   // accumulator tiles per tap
  static constexpr int slab_tiles(int ci) { return ci == 80 ? 54 : 38; }
  static constexpr long slab(int ci) { return (long)slab_tiles(ci) * 1024; }
};

template <typename T, int CI, int ACT, int SUB = 0>
__global__ __launch_bounds__(C64Wg::NTHREADS) void c64_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dA,
                                                                  const T* __restrict__ A, float* __restrict__ partial, int N,
                                                                  int H, int W, int tiles_x, int tiles_per_img, long x_ls,
                                                                  long d_ls, long a_ls, long p_ls, int n_dir) {
  static_assert(SUB == 0 || CI == 64, "the stride-2 view belongs to the 64-channel upconvs");
  typedef C64Wg G;
  typedef typename FragOf<T>::type FragT;
  constexpr int TR = G::rows<T>(), XW = G::xw(CI), RSX = G::rsx<T>(CI), RSD = G::rsd<T>(), NCB = XW / 32, NT = G::nt(CI);
  constexpr int XCH = XW / 8;
  x += (size_t)blockIdx.y * x_ls; dA += (size_t)blockIdx.y * d_ls; A += (size_t)blockIdx.y * a_ls;
  partial += (size_t)blockIdx.y * p_ls;
  __shared__ __attribute__((aligned(16))) T XC[TR * G::TS * RSX];
  __shared__ __attribute__((aligned(16))) T DZ[(TR + 2) * G::DW * RSD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int uy = wave / 3, ux = wave - uy * 3;
  const bool bias_wave = CI == 64 && wave == 4;
  f32x16 acc[3][2];
#pragma unroll
  for (int cb = 0; cb < 3; ++cb) { acc[cb][0] = zero16(); acc[cb][1] = zero16(); }
  FragT ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = (T)((lane & 31) == 0 ? 1.f : 0.f);
  const int half = gridDim.x / 2, second = (n_dir > 0 && (int)blockIdx.x >= half) ? 1 : 0;
  const int t_begin = n_dir > 0 ? second * n_dir * tiles_per_img + ((int)blockIdx.x - second * half) : (int)blockIdx.x;
  const int t_end = n_dir > 0 ? (second ? N : n_dir) * tiles_per_img : N * tiles_per_img;
  const int t_step = n_dir > 0 ? half : (int)gridDim.x;
  for (int t = t_begin; t < t_end; t += t_step) {
    const int n = t / tiles_per_img, tile = t - n * tiles_per_img;
    const int ty0 = (tile / tiles_x) * G::TS, tx0 = (tile % tiles_x) * G::TS;
    const T* const xi = x + (size_t)n * H * W * CI;
    const T* const di = dA + (size_t)n * H * W * (SUB ? 256 : 64);
    const T* const ai = A + (size_t)n * H * W * (SUB ? 256 : 64);
#pragma unroll 1
    for (int r0 = 0; r0 < G::TS; r0 += TR) {
      __syncthreads();
      for (int idx = tid; idx < TR * G::TS * XCH; idx += G::NTHREADS) {           // x on the core rows [r0, r0 + TR)
        const int p = idx / XCH, c = idx - p * XCH, py = p / G::TS, px = p - py * G::TS;
        const int Y = ty0 + r0 + py, X = tx0 + px;
        FragT v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (T)0.f;
        if (c * 8 < CI) {
          if (Y < H && X < W) v = *reinterpret_cast<const FragT*>(xi + ((size_t)Y * W + X) * CI + c * 8);
        } else if (CI == 80 && c == 10) {
          v[0] = (T)1.f;                                                          // the ones channel (80): its centre-tap row is db
        }
        *reinterpret_cast<FragT*>(XC + p * RSX + c * 8) = v;
      }
      for (int idx = tid; idx < (TR + 2) * G::DW * 8; idx += G::NTHREADS) {        // dz = dA * act'(A) on those rows + 1-pixel halo
        const int p = idx >> 3, c = idx & 7, py = p / G::DW, px = p - py * G::DW;
        const int Y = ty0 + r0 - 1 + py, X = tx0 - 1 + px;
        FragT z;
#pragma unroll
        for (int j = 0; j < 8; ++j) z[j] = (T)0.f;
        if (Y >= 0 && Y < H && X >= 0 && X < W) {
          const size_t o = SUB ? ((size_t)(2 * Y + ((int)blockIdx.y >> 1)) * (2 * W) + 2 * X + ((int)blockIdx.y & 1)) * 64 + c * 8
                               : ((size_t)Y * W + X) * 64 + c * 8;
          const FragT gv = *reinterpret_cast<const FragT*>(di + o);
          if constexpr (ACT != 0) {
            const FragT av = *reinterpret_cast<const FragT*>(ai + o);
#pragma unroll
            for (int j = 0; j < 8; ++j) z[j] = (T)((float)gv[j] * c3_dact<ACT>((float)av[j]));
          } else {
            z = gv;
          }
        }
        *reinterpret_cast<FragT*>(DZ + p * RSD + c * 8) = z;
      }
      __syncthreads();
#pragma unroll 1
      for (int s = 0; s < TR; ++s) {                                              // k-step s: core row s of this pass, 16 pixels
        auto rowx = [=](int p) { return p * RSX; };
        auto rowd = [=](int p) { return (((p >> 4) + uy) * G::DW + (p & 15) + ux) * RSD; };
        const FragT b0 = tr_frag<T>(DZ, s, lane, rowd), b1 = tr_frag<T>(DZ + 32, s, lane, rowd);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
          const FragT a = tr_frag<T>(XC + 32 * cb, s, lane, rowx);
          acc[cb][0] = mma16<T>(a, b0, acc[cb][0]);
          acc[cb][1] = mma16<T>(a, b1, acc[cb][1]);
        }
        if (bias_wave) {                                                          // (wave-uniform)
          acc[2][0] = mma16<T>(ones, b0, acc[2][0]);
          acc[2][1] = mma16<T>(ones, b1, acc[2][1]);
        }
      }
    }
  }
  float* const out = partial + (size_t)blockIdx.x * G::slab(CI);
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int ob = 0; ob < 2; ++ob) slab_store_tile(out, wave * NT + 2 * cb + ob, acc[cb][ob], lane);
  if (bias_wave) {
    slab_store_tile(out, 36, acc[2][0], lane);
    slab_store_tile(out, 37, acc[2][1], lane);
  }
}

// ---------------------------------------------------------------------------------------------
// flow_warp backward for the gathered first conv, gather form (c3_warp_bwd_kernel at 64 state channels; d flow is c64_warp_dflow_kernel's): g = the state
// part of dx0 [N][H][W][64];  d state[s] = sum over output pixels o that sampled s of w_tap(o) g[o], each source pixel walking the
// window |o - s| <= ceil(bound) + 1 in a fixed order (no atomics: deterministic).  One thread per source pixel and 16-channel
// group: grid = (tiles, N, 4), 16 fp32 accumulators per thread.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void c64_warp_bwd_kernel(const T* __restrict__ g, const float* __restrict__ flow, long flow_bs,
                                                         const float* __restrict__ flow_bound, T* __restrict__ dstate, int H,
                                                         int W, int tiles_x) {
  typedef typename FragOf<T>::type FragT;
  typedef C3WarpBwd B;
  __shared__ int2 tap_xy[B::NCAND];                  // (x0, y0) of every candidate output pixel; x0 = INT_MIN: outside the image
  __shared__ float2 tap_w[B::NCAND];                 // (wx, wy)
  const int n = blockIdx.y, tile = blockIdx.x, cg = blockIdx.z * 16;
  const int ty0 = (tile / tiles_x) * B::TS, tx0 = (tile % tiles_x) * B::TS;
  const int sy = ty0 + (int)threadIdx.x / B::TS, sx = tx0 + (int)threadIdx.x % B::TS;
  int rw = 0;
  if (flow) {
    const float b = *flow_bound;
    rw = (b < 0.f ? 0 : (b > 1e6f ? 1000000 : (int)ceilf(b))) + 1;
  }
  const bool in_lds = rw <= B::RW_LDS;                // uniform over the grid
  const int cw = B::TS + 2 * rw;
  if (in_lds) {
    for (int i = threadIdx.x; i < cw * cw; i += 256) {
      const int oy = ty0 - rw + i / cw, ox = tx0 - rw + i % cw;
      int2 xy = {INT_MIN, 0};
      float2 wq = {0.f, 0.f};
      if (oy >= 0 && oy < H && ox >= 0 && ox < W) {
        const WarpTaps t = c3_taps_of(flow, flow_bs, n, oy, ox, H, W);
        xy.x = t.x0; xy.y = t.y0; wq.x = t.wx; wq.y = t.wy;
      }
      tap_xy[i] = xy;
      tap_w[i] = wq;
    }
    __syncthreads();
  }
  if (sy >= H || sx >= W) return;
  const T* gi = g + (size_t)n * H * W * 64 + cg;
  float acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0.f;
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
        const WarpTaps t = c3_taps_of(flow, flow_bs, n, oy, ox, H, W);
        x0 = t.x0; y0 = t.y0; wx = t.wx; wy = t.wy;
      }
      const int dy = sy - y0, dx = sx - x0;
      if (dy < 0 || dy > 1 || dx < 0 || dx > 1) continue;
      const float wgt = (dx ? wx : 1.f - wx) * (dy ? wy : 1.f - wy);
      const T* row = gi + ((size_t)oy * W + ox) * 64;
      const FragT q0 = *reinterpret_cast<const FragT*>(row), q1 = *reinterpret_cast<const FragT*>(row + 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) { acc[j] += wgt * (float)q0[j]; acc[8 + j] += wgt * (float)q1[j]; }
    }
  FragT o0, o1;
#pragma unroll
  for (int j = 0; j < 8; ++j) { o0[j] = (T)acc[j]; o1[j] = (T)acc[8 + j]; }
  T* dst = dstate + ((size_t)n * H * W + (size_t)sy * W + sx) * 64 + cg;
  *reinterpret_cast<FragT*>(dst) = o0;
  *reinterpret_cast<FragT*>(dst + 8) = o1;
}

// ---------------------------------------------------------------------------------------------
// flow gradient of the gathered first conv (the opt-in flow_training route): for every output pixel o
//   d flow[o] = sum_c g[o][c] * d(bilinear(state, pos(o)))/d(pos),
// g = the state part of dx0 [N][H][W][64], state = the previous step's NHWC image.  pos(o) and the four taps are c3_taps_of's, the
// function the forward gather calls, so floor and weights are the forward's bit for bit; the derivative is the d flow branch of
// c3_warp_bwd_kernel (conv3x3.h).  A corner outside the image contributes 0 and is never dereferenced.
// Eight lanes per pixel, lane q owning channels 8q..8q+7 of g[o] and of the four corner rows (one 16-byte load each in bf16, 32 in
// fp32); fp32 partials, summed over j = 0..7 in the lane and then over the lanes with __shfl_xor 1, 2, 4: no LDS, no atomics, one
// summation order.  Channels >= num_feat of g and of the state are exactly zero on this route, so no channel count is passed.
// grid = (ceil(H W / 32), N), 256 threads = 32 pixels.  dflow: fp32 [N][2][H][W] planes, batch stride dflow_bs, written (not added to).
// ---------------------------------------------------------------------------------------------
struct C64Dflow {
  static constexpr int NTHREADS = 256, PX = NTHREADS / 8;       // pixels per workgroup
};

template <typename T>
__global__ __launch_bounds__(C64Dflow::NTHREADS) void c64_warp_dflow_kernel(const T* __restrict__ g, const T* __restrict__ state,
                                                                          const float* __restrict__ flow, long flow_bs,
                                                                          float* __restrict__ dflow, long dflow_bs, int H, int W) {
  typedef typename FragOf<T>::type FragT;
  const int n = blockIdx.y, q = threadIdx.x & 7;
  const int plane = H * W, p = blockIdx.x * C64Dflow::PX + ((int)threadIdx.x >> 3);
  const bool live = p < plane;                       // dead lanes load nothing and still take part in the shuffles
  float gx = 0.f, gy = 0.f;
  if (live) {
    const int y = p / W, x = p - y * W;
    const WarpTaps t = c3_taps_of(flow, flow_bs, n, y, x, H, W);
    const bool b00 = t.vy0 && t.vx0, b01 = t.vy0 && t.vx1, b10 = t.vy1 && t.vx0, b11 = t.vy1 && t.vx1;
    if (b00 || b01 || b10 || b11) {
      // 64-bit pixel offset: x0 / y0 of an invalid corner may be anything an int holds
      const long o00 = (long)t.y0 * W + t.x0;
      const T* st = state + ((size_t)n * plane) * 64 + q * 8;
      FragT gv = *reinterpret_cast<const FragT*>(g + ((size_t)n * plane + p) * 64 + q * 8);
      FragT a, b, c, d;
#pragma unroll
      for (int j = 0; j < 8; ++j) { a[j] = (T)0.f; b[j] = (T)0.f; c[j] = (T)0.f; d[j] = (T)0.f; }
      if (b00) a = *reinterpret_cast<const FragT*>(st + o00 * 64);
      if (b01) b = *reinterpret_cast<const FragT*>(st + (o00 + 1) * 64);
      if (b10) c = *reinterpret_cast<const FragT*>(st + (o00 + W) * 64);
      if (b11) d = *reinterpret_cast<const FragT*>(st + (o00 + W + 1) * 64);
      const float uy = 1.f - t.wy, ux = 1.f - t.wx;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float gg = (float)gv[j], v00 = (float)a[j], v01 = (float)b[j], v10 = (float)c[j], v11 = (float)d[j];
        gx += gg * ((v01 - v00) * uy + (v11 - v10) * t.wy);
        gy += gg * ((v10 - v00) * ux + (v11 - v01) * t.wx);
      }
    }
  }
  gx += __shfl_xor(gx, 1); gy += __shfl_xor(gy, 1);
  gx += __shfl_xor(gx, 2); gy += __shfl_xor(gy, 2);
  gx += __shfl_xor(gx, 4); gy += __shfl_xor(gy, 4);
  if (live && q == 0) {
    // d(position)/d(flow) is 1 along an axis of size > 1 and 0 along an axis of size 1 (flow_warp.h)
    float* df = dflow + (size_t)n * dflow_bs + p;
    df[0] = W > 1 ? gx : 0.f;
    df[(size_t)plane] = H > 1 ? gy : 0.f;
  }
}
