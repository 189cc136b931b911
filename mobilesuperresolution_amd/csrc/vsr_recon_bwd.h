// Reconstruction of BasicVSR_origin, the backward of the opt-in training route (gfx950).  Reference ops
// differentiated (models/basicvsr_arch_origin.py:84-93): fusion (1x1) + lrelu, upconv1 / upconv2 (3x3, 64 -> 256) + PixelShuffle(2)
// + lrelu, conv_hr + lrelu, conv_last; the bilinear base has no parameters and the frame takes no gradient.
//
// g = d loss / d out, [N][3][4H][4W] fp32.  Stored gradient images (hot dtype, one rounding each):
//   d_hr    = conv_last^T(g) * lrelu'(hr)                     vr_last_bwd_kernel (VALU: 27 products per element, memory-bound)
//   d_up2   = conv_hr^T(d_hr)                                 c64_conv_kernel<DZ = 0> on the transposed blob (conv64.h)
//   d_up1   = sum_q upconv2_q^T(dz_q), dz_q = (d_up2 * lrelu'(up2)) at pixels (2Y + dy, 2X + dx)      vr_upconv_bwd_kernel
//   d_fused = sum_q upconv1_q^T(dz_q), dz_q from d_up1, up1    vr_upconv_bwd_kernel
//   d state = Wfu^T (d_fused * lrelu'(fused)), one image per trunk: c64_conv_kernel<DZ = 2> on a blob whose centre tap alone is
//             nonzero (a 1x1 conv is that 3x3 conv; at H x W the eight idle taps cost 5 % of the backward's MFMA work)
// Parameter gradients, one fp32 slab per workgroup, plain stores, summed in workgroup order by vr_reduce_kernel:
//   conv_last  vr_last_wgrad_kernel
//   conv_hr    c64_wgrad_kernel<T, 64, none>
//   upconv1/2  c64_wgrad_kernel<T, 64, LeakyReLU, SUB = 1>: blockIdx.y = sub-conv q, dz staged through the stride-2 view
//   fusion     c64_wgrad_kernel<T, 64, LeakyReLU> against each trunk's state image (the centre tap's matrix is dW_fu's half)
// No kernel allocates, synchronises the device or uses a float atomic.
#pragma once
#include "conv64_bwd.h"
#include "vsr_recon.h"

struct VRBwd {
  static constexpr int NSEC = 11;                       // weight-gradient sections: fusion b | f, upconv1 q 0..3, upconv2 q 0..3, conv_hr
  static constexpr int WSLAB = (int)C64Wg::slab(64);    // 38 912 floats
  static constexpr int LAST_W = 27 * 64;                // dW_last as [co][tap][ci]
  static constexpr int LAST_SLAB = LAST_W + 64;         // | db_last [3] | zeros
  static constexpr long per_wg() { return (long)NSEC * WSLAB + LAST_SLAB; }
};

// g on the tile + 1-pixel halo, three planes of 18 x 18, zero outside the image
SR_DEV void vr_stage_g(float* gs, const float* __restrict__ g, int H, int W, int ty0, int tx0, int tid, int nthreads) {
  for (int i = tid; i < 3 * C64Cfg::NPXH; i += nthreads) {
    const int c = i / C64Cfg::NPXH, p = i - c * C64Cfg::NPXH, py = p / C64Cfg::HW, px = p - py * C64Cfg::HW;
    const int Y = ty0 - 1 + py, X = tx0 - 1 + px;
    gs[i] = (Y >= 0 && Y < H && X >= 0 && X < W) ? g[((size_t)c * H + Y) * W + X] : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------
// d_hr[ci, p] = lrelu'(hr[ci, p]) * sum over co, (ky, kx) of W[co, ci, ky, kx] g[co, p - (ky - 1, kx - 1)].  H, W = the x4 size.
// grid = (tiles, N); thread = one pixel of the 16 x 16 tile and one half of its 64 channels.  wl = [co][tap][ci] in the hot dtype.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(C64Cfg::NTHREADS) void vr_last_bwd_kernel(const float* __restrict__ g, long g_bs, const T* __restrict__ hr,
                                                                     const T* __restrict__ wl, T* __restrict__ dhr, int H, int W,
                                                                     int tiles_x) {
  typedef C64Cfg C;
  typedef typename FragOf<T>::type FragT;
  __shared__ float gs[3 * C::NPXH];
  __shared__ __attribute__((aligned(16))) float ws[VRBwd::LAST_W];
  const int tid = threadIdx.x, n = blockIdx.y, tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * C::TH, tx0 = (tile % tiles_x) * C::TW;
  for (int i = tid; i < VRBwd::LAST_W; i += C::NTHREADS) ws[i] = (float)wl[i];
  vr_stage_g(gs, g + (size_t)n * g_bs, H, W, ty0, tx0, tid, C::NTHREADS);
  __syncthreads();
  const int p = tid >> 1, half = tid & 1, oy = p / C::TW, ox = p - oy * C::TW;
  const int Y = ty0 + oy, X = tx0 + ox;
  if (Y >= H || X >= W) return;
  float acc[32];
#pragma unroll
  for (int c = 0; c < 32; ++c) acc[c] = 0.f;
#pragma unroll 1
  for (int k = 0; k < 27; ++k) {
    const int co = k / 9, tap = k - co * 9, ky = tap / 3, kx = tap - ky * 3;
    const float gv = gs[co * C::NPXH + (oy + 2 - ky) * C::HW + ox + 2 - kx];
    const float4* const wr = reinterpret_cast<const float4*>(ws + k * 64 + half * 32);
#pragma unroll
    for (int c4 = 0; c4 < 8; ++c4) {
      const float4 wv = wr[c4];
      acc[4 * c4 + 0] += gv * wv.x; acc[4 * c4 + 1] += gv * wv.y; acc[4 * c4 + 2] += gv * wv.z; acc[4 * c4 + 3] += gv * wv.w;
    }
  }
  const size_t o = (((size_t)n * H + Y) * W + X) * C::CO + half * 32;
#pragma unroll
  for (int c8 = 0; c8 < 4; ++c8) {
    const FragT av = *reinterpret_cast<const FragT*>(hr + o + c8 * 8);
    FragT v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (T)(acc[c8 * 8 + j] * c3_dact<2>((float)av[j]));
    *reinterpret_cast<FragT*>(dhr + o + c8 * 8) = v;
  }
}

// ---------------------------------------------------------------------------------------------
// dW_last[co, ci, ky, kx] = sum over pixels s of g[co, s - (ky - 1, kx - 1)] hr[ci, s], db_last[co] = sum of g[co, s].
// grid = (wgs); a workgroup walks tiles blockIdx.x, + gridDim.x, ...; thread = channel ci = tid & 63, wave v = tile rows 2v, 2v + 1,
// 27 + 1 accumulators; the eight waves' sums are added in wave order through LDS and leave ONE slab [28][64] per workgroup.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(C64Cfg::NTHREADS) void vr_last_wgrad_kernel(const float* __restrict__ g, long g_bs, const T* __restrict__ hr,
                                                                       float* __restrict__ partial, int N, int H, int W, int tiles_x,
                                                                       int tiles_per_img) {
  typedef C64Cfg C;
  __shared__ float gs[3 * C::NPXH];
  __shared__ float red[C::NWAVES * 28 * 64];
  const int tid = threadIdx.x, c = tid & 63, wave = tid >> 6;
  float acc[28];
#pragma unroll
  for (int k = 0; k < 28; ++k) acc[k] = 0.f;
  for (int t = blockIdx.x; t < N * tiles_per_img; t += gridDim.x) {
    const int n = t / tiles_per_img, tile = t - n * tiles_per_img;
    const int ty0 = (tile / tiles_x) * C::TH, tx0 = (tile % tiles_x) * C::TW;
    __syncthreads();
    vr_stage_g(gs, g + (size_t)n * g_bs, H, W, ty0, tx0, tid, C::NTHREADS);
    __syncthreads();
#pragma unroll 1
    for (int pp = 0; pp < 2 * C::TW; ++pp) {
      const int oy = 2 * wave + pp / C::TW, ox = pp % C::TW;
      const int Y = ty0 + oy, X = tx0 + ox;
      if (Y >= H || X >= W) continue;                  // (wave-uniform)
      const float v = (float)hr[(((size_t)n * H + Y) * W + X) * C::CO + c];
#pragma unroll
      for (int k = 0; k < 27; ++k) {
        const int co = k / 9, tap = k - co * 9, ky = tap / 3, kx = tap - ky * 3;
        acc[k] += gs[co * C::NPXH + (oy + 2 - ky) * C::HW + ox + 2 - kx] * v;
      }
      acc[27] += c < 3 ? gs[c * C::NPXH + (oy + 1) * C::HW + ox + 1] : 0.f;
    }
  }
#pragma unroll
  for (int k = 0; k < 28; ++k) red[(wave * 28 + k) * 64 + c] = acc[k];
  __syncthreads();
  float* const out = partial + (size_t)blockIdx.x * VRBwd::LAST_SLAB;
  for (int i = tid; i < VRBwd::LAST_SLAB; i += C::NTHREADS) {
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < C::NWAVES; ++v) s += red[v * 28 * 64 + i];
    out[i] = s;
  }
}

// ---------------------------------------------------------------------------------------------
// backward-data of upconv + PixelShuffle(2) + LeakyReLU: g, a [N][2H][2W][64] (the gradient at the layer's output and the stored
// output) -> dx [N][H][W][64] = sum over q = 2 dy + dx of conv_q^T(dz_q), dz_q[Y, X] = g * lrelu'(a) at (2Y + dy, 2X + dx).
// wblob = four transposed sub-conv blobs (c64_bwd_tables' construction, zero bias).  One 18 x 18 x 64 plane in LDS at a time: the
// loop over q goes around stage + MFMA, the accumulators of the wave's two pixel tiles live across it (fp32, one rounding at the
// store).  grid = (tiles of the H x W image, N)
// ---------------------------------------------------------------------------------------------
template <typename T>
SR_DEV void vr_stage_dz_sub(T* dst, const T* __restrict__ g, const T* __restrict__ a, int H, int W, int y0, int x0, int dy, int dx,
                            int tid) {
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
      const size_t o = ((size_t)(2 * Y + dy) * (2 * W) + 2 * X + dx) * C::CO + c * 8;
      const FragT gv = *reinterpret_cast<const FragT*>(g + o), av = *reinterpret_cast<const FragT*>(a + o);
#pragma unroll
      for (int j = 0; j < 8; ++j) z[j] = (T)((float)gv[j] * c3_dact<2>((float)av[j]));
    }
    *reinterpret_cast<FragT*>(dst + p * RS + c * 8) = z;
  }
}

template <typename T>
__global__ __launch_bounds__(C64Cfg::NTHREADS) void vr_upconv_bwd_kernel(const T* __restrict__ g, const T* __restrict__ a,
                                                                       T* __restrict__ dx, const T* __restrict__ wblob, int H, int W,
                                                                       int tiles_x) {
  typedef C64Cfg C;
  constexpr int RS = C::rs<T>(64), KS = C::ks(64);
  __shared__ __attribute__((aligned(16))) T xs[C::NPXH * RS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5, ch = wave & 1;
  const int n = blockIdx.y, tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * C::TH, tx0 = (tile % tiles_x) * C::TW;
  const size_t img2 = (size_t)n * 4 * H * W * C::CO;
  const int pc0 = (wave >> 1) * 32 + r, pc1 = pc0 + 4 * 32;
  const int oy0 = pc0 / C::TW, ox0 = pc0 - oy0 * C::TW, oy1 = pc1 / C::TW, ox1 = pc1 - oy1 * C::TW;
  f32x16 acc0 = zero16(), acc1 = zero16();
  C64W<T, KS> w;
#pragma unroll 1
  for (int q = 0; q < 4; ++q) {
    if (q > 0) __syncthreads();                        // every wave has read plane q - 1
    w.load(wblob + (size_t)q * VRCfg::SUB_ELEMS, ch, lane);
    vr_stage_dz_sub<T>(xs, g + img2, a + img2, H, W, ty0 - 1, tx0 - 1, q >> 1, q & 1, tid);
    __syncthreads();
    acc0 = c64_mma<T, 64, KS>(xs, (oy0 * C::HW + ox0) * RS, C::HW, w, acc0, lane);
    acc1 = c64_mma<T, 64, KS>(xs, (oy1 * C::HW + ox1) * RS, C::HW, w, acc1, lane);
  }
  const int Y0 = ty0 + oy0, X0 = tx0 + ox0, Y1 = ty0 + oy1, X1 = tx0 + ox1;
  if (Y0 < H && X0 < W) vr_store_half<T, 0>(dx + (((size_t)n * H + Y0) * W + X0) * C::CO + 32 * ch + 4 * hh, acc0);
  if (Y1 < H && X1 < W) vr_store_half<T, 0>(dx + (((size_t)n * H + Y1) * W + X1) * C::CO + 32 * ch + 4 * hh, acc1);
}

// ---------------------------------------------------------------------------------------------
// slab reduction: grads[i] (+)= sum over the section's workgroups w = 0 .. e - 1, in that order, of the slab element table[i] names
// (e = e0 for the sections summed over the H x W image, k < 6; e1 at 2H x 2W, k < 10; e2 at 4H x 4W).
// table[i] = k * WSLAB + e: element e of section k's slab (k < NSEC: parts + (k wgs + w) WSLAB; k = NSEC: conv_last's slabs behind
// them, LAST_SLAB floats each).  packing.c64_recon_bwd_tables(F)["reduce"].
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vr_reduce_kernel(const float* __restrict__ parts, const int* __restrict__ table,
                                                      float* __restrict__ grads, int n, int wgs, int e0, int e1, int e2, int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int v = table[i], k = v / VRBwd::WSLAB, e = v - k * VRBwd::WSLAB;
  const long stride = k < VRBwd::NSEC ? VRBwd::WSLAB : VRBwd::LAST_SLAB;
  const float* p = parts + (size_t)k * wgs * VRBwd::WSLAB + e;
  float s = 0.f;
  const int ne = k < 6 ? e0 : (k < 10 ? e1 : e2);
  for (int w = 0; w < ne; ++w) s += p[(size_t)w * stride];
  grads[i] = accumulate ? grads[i] + s : s;
}
