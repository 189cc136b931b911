// Reconstruction of MotionVectorVSR, forward and backward (gfx950).  Reference ops replaced (models/mvvsr_arch.py:95-105), per frame:
//   u = lrelu_0.1(fusion(cat[feat_b, feat_f]));  D = conv_last(u)  (ConvTranspose2d(2F, 3, 5, stride = 4) -> (4h + 1) x (4w + 1));
//   out = interpolate(D, (4h, 4w), 'bilinear') + interpolate(x_i, (4h, 4w), 'bilinear')
// Two laws make it gather-only (tests/mv_recon_ref.py states and checks them in float64):
//   phase form   D[o, 4y + i, 4x + j] = b[o] + E[o,i,j](y, x) + [i = 0] E[o,4,j](y-1, x) + [j = 0] E[o,i,4](y, x-1)
//                + [i = j = 0] E[o,4,4](y-1, x-1), with E[o,ky,kx](y, x) = sum_c u[c,y,x] W[c,o,ky,kx] (75 rows per LR pixel, a dense
//                1x1 contraction) and u = 0 outside the image;
//   resize       (4h + 1) -> 4h is the fixed two-tap blend out[d] = (1 - l_d) D[d] + l_d D[d + 1], l_d = (2d + 1) / (8h), never clamped.
// Layout: the two trunks' NHWC state images (cw = 24 or 64 channels per pixel, channels >= F exactly zero) are read directly; the
// kernel channel of cat channel c is c (c < F) or cw + c - F; u keeps 2 cw channels, channel c of fusion's output at c.
// MFMA: v_mfma_f32_16x16x32_bf16 (fp32 parity: 8 x v_mfma_f32_16x16x4_f32) through vr_mma32 of vsr_recon.h: weights as the A operand
// (lane l: row l & 15, k = 8 (l >> 4) + j), 16 pixels as B; accumulator reg i of lane l = row 4 (l >> 4) + i of pixel l & 15.
//
//   mv_recon_fwd_kernel   one workgroup = one TH x 16 LR tile of one frame of one clip: stage cat with a 1-pixel halo -> fusion + LeakyReLU
//                         in place (u, optionally saved) -> E (fp32, LDS) -> D tile (fp32, LDS; D never goes to memory) -> blend + x4
//                         bilinear base -> NCHW fp32 into the caller's (b, n, 3, 4h, 4w) tensor.
//   mv_recon_bwd_kernel   cw = 24.  Workgroups walk the tiles of the whole clip: dD (the blend's transpose, a gather of 4 output
//                         gradients) -> du = W dE (dE = the 75 dD values of an LR pixel) -> dpre = du lrelu'(u) -> dc = Wfu^T dpre ->
//                         the two state gradients (NHWC, hot dtype); the parameter gradients contract over the tile's pixels into
//                         accumulators kept across tiles and leave as ONE fp32 slab per workgroup.
//   mv_recon_reduce_kernel  sums the slabs in a fixed order into the four parameter gradients (reference shapes).  No atomics anywhere.
#pragma once
#include "vsr_recon.h"

template <typename T, int CW> struct MVCfg {
  static constexpr int NT = 256, NW = 4, TW = 16;
  static constexpr int TH = (sizeof(T) == 4 && CW == 64) ? 4 : 8;          // fp32 at 128 channels: a smaller tile fits the LDS
  static constexpr int HH = TH + 2, HWD = TW + 2, NPH = HH * HWD, NG = (NPH + 15) / 16, NPHP = NG * 16;
  static constexpr int KC = 2 * CW, KP = (KC + 31) / 32 * 32, KS = KP / 32, MB = KP / 16, RS = KP + 8;
  static constexpr int NE = 80, EB = 5, ERS = 84;                          // E rows r = o 25 + ky 5 + kx (75 real)
  static constexpr int DH = 4 * TH + 1, DW = 4 * TW + 1, ND = 3 * DH * DW;
  static constexpr int NPC = TH * TW;                                      // core pixels
  // packed blob (packing.mv_recon_tables): forward | backward (cw = 24 only)
  static constexpr int OFF_BFU = MB * KS * 512, OFF_WL = OFF_BFU + KP, OFF_BL = OFF_WL + EB * KS * 512, FWD_ELEMS = OFF_BL + 8;
  static constexpr int KSB = 3;                                            // 96 = 75 padded / 32
  static constexpr int OFF_WLB = FWD_ELEMS, OFF_WFUT = OFF_WLB + MB * KSB * 512, ALL_ELEMS = OFF_WFUT + MB * KS * 512;
  // one workgroup's slab of parameter gradients: dW_last [64][80] | dW_fu [64][64] (column 48 = db_fu) | db_last [3] | pad
  static constexpr int SLAB_WL = 0, SLAB_WFU = 64 * 80, SLAB_BL = SLAB_WFU + 64 * 64, SLAB = SLAB_BL + 16;
  // cw = 64: the backward has a blob of its own (packing.mv_recon_bwd_tables): wlb | wfut
  static constexpr int B64_WLB = 0, B64_WFUT = MB * KSB * 512, B64_ELEMS = B64_WFUT + MB * KS * 512;
  // and its slab: dW_last [128][80] | dW_fu [128][128] | db_fu [128] | db_last [3] | pad
  static constexpr int S64_WL = 0, S64_WFU = 128 * 80, S64_BFU = S64_WFU + 128 * 128, S64_BL = S64_BFU + 128, SLAB64 = S64_BL + 16;
};

struct MVPtrs { const void* fb[16]; const void* ff[16]; };
struct MVGPtrs { void* dfb[16]; void* dff[16]; };

// blend weight of D row d + 1 at output row d, as ATen's upsample_bilinear2d computes it (scale = (4h + 1) / 4h in fp32,
// src = scale (d + 0.5) - 0.5); the integer part of src is d
SR_DEV float mv_lambda(int d, float scale) {
  const float l = scale * ((float)d + 0.5f) - 0.5f - (float)d;
  return fminf(fmaxf(l, 0.f), 1.f);
}

template <typename T, int CW>
__global__ __launch_bounds__(256) void mv_recon_fwd_kernel(MVPtrs ptrs, const T* __restrict__ blob, const float* __restrict__ x,
                                                           long x_bs, long x_fs, float* __restrict__ out, long out_bs, long out_fs,
                                                           T* __restrict__ usave, int f0, int B, int H, int W, int tiles_x) {
  typedef MVCfg<T, CW> C;
  typedef typename FragOf<T>::type FragT;
  typedef typename FragOf<T>::half_type HalfT;
  constexpr int CS_BYTES = C::NPHP * C::RS * (int)sizeof(T), D_BYTES = C::ND * 4;
  constexpr int A_BYTES = ((CS_BYTES > D_BYTES ? CS_BYTES : D_BYTES) + 31) / 32 * 32;
  __shared__ __attribute__((aligned(32))) unsigned char smem[A_BYTES + C::NPH * C::ERS * 4];
  T* const cs = reinterpret_cast<T*>(smem);                  // cat, then u in place
  float* const ds = reinterpret_cast<float*>(smem);          // the D tile, once u is dead
  float* const es = reinterpret_cast<float*>(smem + A_BYTES);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, q = lane >> 4;
  const int n = blockIdx.y, fz = blockIdx.z, tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * C::TH, tx0 = (tile % tiles_x) * C::TW;
  const T* const fb = reinterpret_cast<const T*>(ptrs.fb[fz]) + (size_t)n * H * W * CW;
  const T* const ff = reinterpret_cast<const T*>(ptrs.ff[fz]) + (size_t)n * H * W * CW;
  constexpr int CPR = C::KP / 8, CPS = CW / 8;
  for (int idx = tid; idx < C::NPHP * CPR; idx += C::NT) {
    const int p = idx / CPR, cc = idx - p * CPR;
    const int hy = p / C::HWD, hx = p - hy * C::HWD;
    const int Y = ty0 - 1 + hy, X = tx0 - 1 + hx;
    FragT v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (T)0.f;
    if (p < C::NPH && Y >= 0 && Y < H && X >= 0 && X < W && cc < 2 * CPS) {
      const T* const src = cc < CPS ? fb : ff;
      v = *reinterpret_cast<const FragT*>(src + ((size_t)Y * W + X) * CW + (cc < CPS ? cc : cc - CPS) * 8);
    }
    *reinterpret_cast<FragT*>(cs + p * C::RS + cc * 8) = v;
  }
  __syncthreads();
  T* const us = usave ? usave + ((size_t)(f0 + fz) * B + n) * H * W * C::KC : nullptr;
#pragma unroll 1
  for (int g = wave; g < C::NG; g += C::NW) {
    const int p = g * 16 + l16;
    const int hy = p / C::HWD, hx = p - hy * C::HWD;
    const int Y = ty0 - 1 + hy, X = tx0 - 1 + hx;
    const bool in = p < C::NPH && Y >= 0 && Y < H && X >= 0 && X < W;
    const bool core = in && hy >= 1 && hy <= C::TH && hx >= 1 && hx <= C::TW;
    // the weight fragments stay inside the loops (laundered base): hoisted, the 128-channel fp32 set alone is 256 registers
    FragT bc[C::KS];
#pragma unroll
    for (int s = 0; s < C::KS; ++s) bc[s] = lds_chunk<T>(cs, p * C::RS + 32 * s + 8 * q);
#pragma unroll 1
    for (int mh = 0; mh < C::MB; mh += 4) {
      const T* const wf = weights_for_tile<false>(blob);
      f32x4 acc[4];
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[m][i] = (float)wf[C::OFF_BFU + 16 * (mh + m) + 4 * q + i];
#pragma unroll
      for (int s = 0; s < C::KS; ++s)
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[m] = vr_mma32<T>(load_wfrag<T>(wf, (mh + m) * C::KS + s, lane), bc[s], acc[m]);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int ch = 16 * (mh + m) + 4 * q;
        HalfT v;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float t = acc[m][i];
          v[i] = in ? (T)(t > 0.f ? t : 0.1f * t) : (T)0.f;     // u is ZERO outside the image (not lrelu(bias))
        }
        *reinterpret_cast<HalfT*>(cs + p * C::RS + ch) = v;     // in place: this wave has read all of its 16 rows (bc)
        if (us && core && ch < C::KC) *reinterpret_cast<HalfT*>(us + ((size_t)Y * W + X) * C::KC + ch) = v;
      }
    }
#pragma unroll
    for (int s = 0; s < C::KS; ++s) bc[s] = lds_chunk<T>(cs, p * C::RS + 32 * s + 8 * q);
#pragma unroll 1
    for (int eb = 0; eb < C::EB; ++eb) {
      const T* const wf = weights_for_tile<false>(blob + C::OFF_WL);
      f32x4 e = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < C::KS; ++s) e = vr_mma32<T>(load_wfrag<T>(wf, eb * C::KS + s, lane), bc[s], e);
      if (p < C::NPH) *reinterpret_cast<f32x4*>(es + p * C::ERS + 16 * eb + 4 * q) = e;
    }
  }
  __syncthreads();
  const float b0 = (float)blob[C::OFF_BL], b1 = (float)blob[C::OFF_BL + 1], b2 = (float)blob[C::OFF_BL + 2];
  for (int idx = tid; idx < C::ND; idx += C::NT) {
    const int o = idx / (C::DH * C::DW), rem = idx - o * (C::DH * C::DW);
    const int dy = rem / C::DW, dx = rem - dy * C::DW;
    const int ly = dy >> 2, i = dy & 3, lx = dx >> 2, j = dx & 3;
    const int p = (ly + 1) * C::HWD + lx + 1;
    float v = (o == 0 ? b0 : o == 1 ? b1 : b2) + es[p * C::ERS + o * 25 + i * 5 + j];
    if (i == 0) v += es[(p - C::HWD) * C::ERS + o * 25 + 20 + j];
    if (j == 0) v += es[(p - 1) * C::ERS + o * 25 + i * 5 + 4];
    if (i == 0 && j == 0) v += es[(p - C::HWD - 1) * C::ERS + o * 25 + 24];
    ds[idx] = v;
  }
  __syncthreads();
  const int H4 = 4 * H, W4 = 4 * W;
  const float sy = (float)(H4 + 1) / (float)H4, sx = (float)(W4 + 1) / (float)W4;
  float* const o_ = out + (size_t)n * out_bs + (size_t)(f0 + fz) * out_fs;
  const float* const fr = x + (size_t)n * x_bs + (size_t)(f0 + fz) * x_fs;
  for (int idx = tid; idx < 16 * C::TH * C::TW; idx += C::NT) {
    const int oy = idx / (4 * C::TW), ox = idx - oy * (4 * C::TW);
    const int Y = 4 * ty0 + oy, X = 4 * tx0 + ox;
    if (Y < H4 && X < W4) {
      const float ly = mv_lambda(Y, sy), lx = mv_lambda(X, sx);
      const VRTap ty = vr_tap(Y, H), tx = vr_tap(X, W);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* const d = ds + (c * C::DH + oy) * C::DW + ox;
        const float top = (1.f - lx) * d[0] + lx * d[1], bot = (1.f - lx) * d[C::DW] + lx * d[C::DW + 1];
        o_[((size_t)c * H4 + Y) * W4 + X] = (1.f - ly) * top + ly * bot + vr_base(fr + (size_t)c * H * W, W, ty, tx);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// backward (cw = 24).  grid = wgs workgroups over `items` = frames x B x tiles; slab of workgroup w at parts + w * SLAB
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void mv_recon_bwd_kernel(MVPtrs ptrs, MVGPtrs gptrs, const T* __restrict__ blob,
                                                           const T* __restrict__ usave, const float* __restrict__ gout, long g_bs,
                                                           long g_fs, float* __restrict__ parts, int f0, int nf, int B, int H, int W,
                                                           int tiles_x, int tiles) {
  typedef MVCfg<T, 24> C;
  typedef typename FragOf<T>::type FragT;
  typedef typename FragOf<T>::half_type HalfT;
  constexpr int IMG = C::NPC * C::RS;
  __shared__ __attribute__((aligned(32))) float dd[C::ND + 5];               // the dD tile; afterwards the db_last reduction
  __shared__ __attribute__((aligned(32))) T us[IMG];
  __shared__ __attribute__((aligned(32))) T cs[IMG];
  __shared__ __attribute__((aligned(32))) T dp[IMG];
  __shared__ int koff[96];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, q = lane >> 4;
  if (tid < 96) koff[tid] = tid < 75 ? ((tid / 25) * C::DH + (tid % 25) / 5) * C::DW + tid % 5 : -1;
  const int H4 = 4 * H, W4 = 4 * W;
  const float sy = (float)(H4 + 1) / (float)H4, sx = (float)(W4 + 1) / (float)W4;
  f32x4 accl[C::EB], accf[4];
#pragma unroll
  for (int e = 0; e < C::EB; ++e) accl[e] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e) accf[e] = f32x4{0.f, 0.f, 0.f, 0.f};
  float gsum[3] = {0.f, 0.f, 0.f};
  const int items = nf * B * tiles;
#pragma unroll 1
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int tile = item % tiles, n = (item / tiles) % B, fz = item / (tiles * B);
    const int ty0 = (tile / tiles_x) * C::TH, tx0 = (tile % tiles_x) * C::TW;
    const size_t img = (size_t)n * H * W;
    const T* const fb = reinterpret_cast<const T*>(ptrs.fb[fz]) + img * 24;
    const T* const ff = reinterpret_cast<const T*>(ptrs.ff[fz]) + img * 24;
    T* const dfb = reinterpret_cast<T*>(gptrs.dfb[fz]) + img * 24;
    T* const dff = reinterpret_cast<T*>(gptrs.dff[fz]) + img * 24;
    const T* const u = usave + ((size_t)(f0 + fz) * B + n) * H * W * C::KC;
    const float* const g = gout + (size_t)n * g_bs + (size_t)(f0 + fz) * g_fs;
    __syncthreads();                                       // the previous tile's readers are done (and koff is written)
    for (int idx = tid; idx < C::NPC * 8; idx += C::NT) {
      const int p = idx >> 3, cc = idx & 7;
      const int Y = ty0 + p / C::TW, X = tx0 + p % C::TW;
      FragT uv, cv;
#pragma unroll
      for (int j = 0; j < 8; ++j) uv[j] = cv[j] = (T)0.f;
      if (Y < H && X < W) {
        const size_t pix = (size_t)Y * W + X;
        if (cc < 6) uv = *reinterpret_cast<const FragT*>(u + pix * C::KC + cc * 8);
        if (cc < 3) cv = *reinterpret_cast<const FragT*>(fb + pix * 24 + cc * 8);
        else if (cc < 6) cv = *reinterpret_cast<const FragT*>(ff + pix * 24 + (cc - 3) * 8);
        else if (cc == 6) cv[0] = (T)1.f;                    // the ones channel: column 48 of dW_fu is db_fu
      }
      *reinterpret_cast<FragT*>(us + p * C::RS + cc * 8) = uv;
      *reinterpret_cast<FragT*>(cs + p * C::RS + cc * 8) = cv;
      if (cc >= 6) *reinterpret_cast<FragT*>(dp + p * C::RS + cc * 8) = uv;      // zero rows 48..63 of dpre
    }
    // db_last = sum of dD = sum of the output gradient (the blend's weights sum to one): this tile's own 4TH x 64 outputs
    for (int idx = tid; idx < 3 * 16 * C::NPC; idx += C::NT) {
      const int o = idx / (16 * C::NPC), rem = idx - o * (16 * C::NPC);
      const int Y = 4 * ty0 + rem / (4 * C::TW), X = 4 * tx0 + rem % (4 * C::TW);
      const float v = (Y < H4 && X < W4) ? g[((size_t)o * H4 + Y) * W4 + X] : 0.f;
      if (o == 0) gsum[0] += v; else if (o == 1) gsum[1] += v; else gsum[2] += v;
    }
    // dD[a][e] = sum over the (at most) four outputs that read it
    for (int idx = tid; idx < C::ND; idx += C::NT) {
      const int o = idx / (C::DH * C::DW), rem = idx - o * (C::DH * C::DW);
      const int dy = rem / C::DW, dx = rem - dy * C::DW;
      const int a = 4 * ty0 + dy, e = 4 * tx0 + dx;
      const float* const go = g + (size_t)o * H4 * W4;
      const float wy0 = a < H4 ? 1.f - mv_lambda(a, sy) : 0.f, wy1 = (a >= 1 && a <= H4) ? mv_lambda(a - 1, sy) : 0.f;
      const float wx0 = e < W4 ? 1.f - mv_lambda(e, sx) : 0.f, wx1 = (e >= 1 && e <= W4) ? mv_lambda(e - 1, sx) : 0.f;
      float v = 0.f;
      if (a < H4) {
        if (e < W4) v += wy0 * wx0 * go[(size_t)a * W4 + e];
        if (e >= 1 && e <= W4) v += wy0 * wx1 * go[(size_t)a * W4 + e - 1];
      }
      if (a >= 1 && a <= H4) {
        if (e < W4) v += wy1 * wx0 * go[(size_t)(a - 1) * W4 + e];
        if (e >= 1 && e <= W4) v += wy1 * wx1 * go[(size_t)(a - 1) * W4 + e - 1];
      }
      dd[idx] = v;
    }
    __syncthreads();
    // du -> dpre -> dc, 16 pixels at a time
#pragma unroll 1
    for (int gq = wave; gq < C::NPC / 16; gq += C::NW) {
      const int p = gq * 16 + l16;
      const int ly = p / C::TW, lx = p % C::TW;
      const int Y = ty0 + ly, X = tx0 + lx;
      const int pixoff = 4 * ly * C::DW + 4 * lx;
      f32x4 du[3];
#pragma unroll
      for (int m = 0; m < 3; ++m) du[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < C::KSB; ++s) {
        FragT b;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int ko = koff[32 * s + 8 * q + j];
          b[j] = (T)(ko >= 0 ? dd[ko + pixoff] : 0.f);
        }
#pragma unroll
        for (int m = 0; m < 3; ++m) du[m] = vr_mma32<T>(load_wfrag<T>(blob + C::OFF_WLB, m * C::KSB + s, lane), b, du[m]);
      }
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        const HalfT uv = *reinterpret_cast<const HalfT*>(us + p * C::RS + 16 * m + 4 * q);
        HalfT v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (T)((float)uv[i] > 0.f ? du[m][i] : 0.1f * du[m][i]);
        *reinterpret_cast<HalfT*>(dp + p * C::RS + 16 * m + 4 * q) = v;
      }
      f32x4 dc[3];
#pragma unroll
      for (int m = 0; m < 3; ++m) dc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < C::KS; ++s) {
        const FragT b = lds_chunk<T>(dp, p * C::RS + 32 * s + 8 * q);
#pragma unroll
        for (int m = 0; m < 3; ++m) dc[m] = vr_mma32<T>(load_wfrag<T>(blob + C::OFF_WFUT, m * C::KS + s, lane), b, dc[m]);
      }
      if (Y < H && X < W) {
        const size_t pix = (size_t)Y * W + X;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
          HalfT v;
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = (T)dc[m][i];
          const int kc = 16 * m + 4 * q;
          T* const dst = kc < 24 ? dfb + pix * 24 + kc : dff + pix * 24 + kc - 24;
          *reinterpret_cast<HalfT*>(dst) = v;
        }
      }
    }
    __syncthreads();
    // parameter gradients: wave m owns rows 16 m .. 16 m + 15 (u channels / fusion outputs); the contraction runs over the tile's pixels
    if (wave < 3) {
      const int row = 16 * wave + l16;
#pragma unroll 1
      for (int s = 0; s < C::NPC / 32; ++s) {
        FragT au, ad;
        int po[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int p = 32 * s + 8 * q + j;
          au[j] = us[p * C::RS + row];
          ad[j] = dp[p * C::RS + row];
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
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
          FragT b;
#pragma unroll
          for (int j = 0; j < 8; ++j) b[j] = cs[(32 * s + 8 * q + j) * C::RS + 16 * nb + l16];
          accf[nb] = vr_mma32<T>(ad, b, accf[nb]);
        }
      }
    }
  }
  float* const slab = parts + (size_t)blockIdx.x * C::SLAB;
  if (wave < 3) {
#pragma unroll
    for (int eb = 0; eb < C::EB; ++eb)
#pragma unroll
      for (int i = 0; i < 4; ++i) slab[C::SLAB_WL + (16 * wave + 4 * q + i) * 80 + 16 * eb + l16] = accl[eb][i];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
      for (int i = 0; i < 4; ++i) slab[C::SLAB_WFU + (16 * wave + 4 * q + i) * 64 + 16 * nb + l16] = accf[nb][i];
  }
  __syncthreads();
#pragma unroll
  for (int o = 0; o < 3; ++o) dd[o * C::NT + tid] = gsum[o];
  __syncthreads();
  if (tid < 3) {
    float t = 0.f;
    for (int k = 0; k < C::NT; ++k) t += dd[tid * C::NT + k];
    slab[C::SLAB_BL + tid] = t;
  }
}

// grads = dW_fu (2F, 2F) | db_fu (2F) | dW_last (2F, 3, 5, 5) | db_last (3): slab k of every workgroup, summed in workgroup order
__global__ __launch_bounds__(256) void mv_recon_reduce_kernel(const float* __restrict__ parts, int nslabs, float* __restrict__ grads, int F) {
  typedef MVCfg<float, 24> C;
  const int F2 = 2 * F, n0 = F2 * F2, n1 = n0 + F2, n2 = n1 + F2 * 75, total = n2 + 3;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int off;
  if (i < n0) {
    const int oc = i / F2, ic = i - oc * F2;
    off = C::SLAB_WFU + oc * 64 + (ic < F ? ic : 24 + ic - F);
  } else if (i < n1) {
    off = C::SLAB_WFU + (i - n0) * 64 + 48;
  } else if (i < n2) {
    const int c = (i - n1) / 75, r = (i - n1) - c * 75;
    off = C::SLAB_WL + c * 80 + r;
  } else {
    off = C::SLAB_BL + (i - n2);
  }
  float t = 0.f;
  for (int k = 0; k < nslabs; ++k) t += parts[(size_t)k * C::SLAB + off];
  grads[i] = t;
}

// ---------------------------------------------------------------------------------------------
// backward at cw = 64 (24 < F <= 64): 128 channels, KS = 4, MB = 8; the tile of MVCfg<T, 64> (8 x 16 pixels in bf16, 4 x 16 in fp32,
// the forward's choice) keeps us | cs | dp at RS = 136 plus the dD tile inside the LDS.  Same mathematics, rounding points and item
// walk as mv_recon_bwd_kernel.  What differs:
//   weights      blob = packing.mv_recon_bwd_tables: wlb (8 x 3 fragments) | wfut (8 x 4); the fragments are loaded inside the
//                row-block loops from a laundered base, four row blocks at a time (hoisted, the fp32 set alone is 448 registers)
//   accumulators wave v owns rows 32 v .. 32 v + 31 (u channels of dW_last, fusion outputs of dW_fu): 2 x (5 + 8) tiles + 2 for db_fu
//                = 112 registers, kept across the workgroup's tiles
//   db_fu        there is no spare channel for a ones column at 128 real channels: dpre is contracted with a ones fragment (as
//                c64_wgrad_kernel does at CI = 64); dpre of a pixel outside the image is therefore stored as zero
//   slab         dW_last [128][80] | dW_fu [128][128] | db_fu [128] | db_last [3], every element written by plain stores
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void mv_recon_bwd64_kernel(MVPtrs ptrs, MVGPtrs gptrs, const T* __restrict__ blob,
                                                             const T* __restrict__ usave, const float* __restrict__ gout, long g_bs,
                                                             long g_fs, float* __restrict__ parts, int f0, int nf, int B, int H, int W,
                                                             int tiles_x, int tiles) {
  typedef MVCfg<T, 64> C;
  typedef typename FragOf<T>::type FragT;
  typedef typename FragOf<T>::half_type HalfT;
  constexpr int IMG = C::NPC * C::RS;
  __shared__ __attribute__((aligned(32))) float dd[C::ND + 5];               // the dD tile; afterwards the db_last reduction
  __shared__ __attribute__((aligned(32))) T us[IMG];
  __shared__ __attribute__((aligned(32))) T cs[IMG];
  __shared__ __attribute__((aligned(32))) T dp[IMG];
  __shared__ int koff[96];
  static_assert(C::ND >= 3 * C::NT, "the db_last reduction reuses the dD tile");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, q = lane >> 4;
  if (tid < 96) koff[tid] = tid < 75 ? ((tid / 25) * C::DH + (tid % 25) / 5) * C::DW + tid % 5 : -1;
  const int H4 = 4 * H, W4 = 4 * W;
  const float sy = (float)(H4 + 1) / (float)H4, sx = (float)(W4 + 1) / (float)W4;
  f32x4 accl[2][C::EB], accf[2][C::MB], accb[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
#pragma unroll
    for (int e = 0; e < C::EB; ++e) accl[m][e] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < C::MB; ++e) accf[m][e] = f32x4{0.f, 0.f, 0.f, 0.f};
    accb[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  FragT ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = (T)1.f;
  float gsum[3] = {0.f, 0.f, 0.f};
  const int items = nf * B * tiles;
#pragma unroll 1
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int tile = item % tiles, n = (item / tiles) % B, fz = item / (tiles * B);
    const int ty0 = (tile / tiles_x) * C::TH, tx0 = (tile % tiles_x) * C::TW;
    const size_t img = (size_t)n * H * W;
    const T* const fb = reinterpret_cast<const T*>(ptrs.fb[fz]) + img * 64;
    const T* const ff = reinterpret_cast<const T*>(ptrs.ff[fz]) + img * 64;
    T* const dfb = reinterpret_cast<T*>(gptrs.dfb[fz]) + img * 64;
    T* const dff = reinterpret_cast<T*>(gptrs.dff[fz]) + img * 64;
    const T* const u = usave + ((size_t)(f0 + fz) * B + n) * H * W * C::KC;
    const float* const g = gout + (size_t)n * g_bs + (size_t)(f0 + fz) * g_fs;
    __syncthreads();                                       // the previous tile's readers are done (and koff is written)
    for (int idx = tid; idx < C::NPC * 16; idx += C::NT) {
      const int p = idx >> 4, cc = idx & 15;
      const int Y = ty0 + p / C::TW, X = tx0 + p % C::TW;
      FragT uv, cv;
#pragma unroll
      for (int j = 0; j < 8; ++j) uv[j] = cv[j] = (T)0.f;
      if (Y < H && X < W) {
        const size_t pix = (size_t)Y * W + X;
        uv = *reinterpret_cast<const FragT*>(u + pix * C::KC + cc * 8);
        cv = *reinterpret_cast<const FragT*>((cc < 8 ? fb : ff) + pix * 64 + (cc & 7) * 8);
      }
      *reinterpret_cast<FragT*>(us + p * C::RS + cc * 8) = uv;
      *reinterpret_cast<FragT*>(cs + p * C::RS + cc * 8) = cv;
    }
    // db_last = sum of dD = sum of the output gradient (the blend's weights sum to one): this tile's own 4TH x 64 outputs
    for (int idx = tid; idx < 3 * 16 * C::NPC; idx += C::NT) {
      const int o = idx / (16 * C::NPC), rem = idx - o * (16 * C::NPC);
      const int Y = 4 * ty0 + rem / (4 * C::TW), X = 4 * tx0 + rem % (4 * C::TW);
      const float v = (Y < H4 && X < W4) ? g[((size_t)o * H4 + Y) * W4 + X] : 0.f;
      if (o == 0) gsum[0] += v; else if (o == 1) gsum[1] += v; else gsum[2] += v;
    }
    // dD[a][e] = sum over the (at most) four outputs that read it
    for (int idx = tid; idx < C::ND; idx += C::NT) {
      const int o = idx / (C::DH * C::DW), rem = idx - o * (C::DH * C::DW);
      const int dy = rem / C::DW, dx = rem - dy * C::DW;
      const int a = 4 * ty0 + dy, e = 4 * tx0 + dx;
      const float* const go = g + (size_t)o * H4 * W4;
      const float wy0 = a < H4 ? 1.f - mv_lambda(a, sy) : 0.f, wy1 = (a >= 1 && a <= H4) ? mv_lambda(a - 1, sy) : 0.f;
      const float wx0 = e < W4 ? 1.f - mv_lambda(e, sx) : 0.f, wx1 = (e >= 1 && e <= W4) ? mv_lambda(e - 1, sx) : 0.f;
      float v = 0.f;
      if (a < H4) {
        if (e < W4) v += wy0 * wx0 * go[(size_t)a * W4 + e];
        if (e >= 1 && e <= W4) v += wy0 * wx1 * go[(size_t)a * W4 + e - 1];
      }
      if (a >= 1 && a <= H4) {
        if (e < W4) v += wy1 * wx0 * go[(size_t)(a - 1) * W4 + e];
        if (e >= 1 && e <= W4) v += wy1 * wx1 * go[(size_t)(a - 1) * W4 + e - 1];
      }
      dd[idx] = v;
    }
    __syncthreads();
    // du -> dpre -> dc, 16 pixels at a time, four row blocks of 16 channels at a time
#pragma unroll 1
    for (int gq = wave; gq < C::NPC / 16; gq += C::NW) {
      const int p = gq * 16 + l16;
      const int ly = p / C::TW, lx = p % C::TW;
      const int Y = ty0 + ly, X = tx0 + lx;
      const bool inimg = Y < H && X < W;
      const int pixoff = 4 * ly * C::DW + 4 * lx;
      FragT bd[C::KSB];
#pragma unroll
      for (int s = 0; s < C::KSB; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int ko = koff[32 * s + 8 * q + j];
          bd[s][j] = (T)(ko >= 0 ? dd[ko + pixoff] : 0.f);
        }
#pragma unroll 1
      for (int mh = 0; mh < C::MB; mh += 4) {
        const T* const wf = weights_for_tile<false>(blob + C::B64_WLB);
        f32x4 du[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) du[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < C::KSB; ++s)
#pragma unroll
          for (int m = 0; m < 4; ++m) du[m] = vr_mma32<T>(load_wfrag<T>(wf, (mh + m) * C::KSB + s, lane), bd[s], du[m]);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int ch = 16 * (mh + m) + 4 * q;
          const HalfT uv = *reinterpret_cast<const HalfT*>(us + p * C::RS + ch);
          HalfT v;
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = inimg ? (T)((float)uv[i] > 0.f ? du[m][i] : 0.1f * du[m][i]) : (T)0.f;
          *reinterpret_cast<HalfT*>(dp + p * C::RS + ch) = v;
        }
      }
      FragT bp[C::KS];                                     // this wave's own 16 rows of dpre, all 128 channels written above
#pragma unroll
      for (int s = 0; s < C::KS; ++s) bp[s] = lds_chunk<T>(dp, p * C::RS + 32 * s + 8 * q);
#pragma unroll 1
      for (int mh = 0; mh < C::MB; mh += 4) {
        const T* const wf = weights_for_tile<false>(blob + C::B64_WFUT);
        f32x4 dc[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) dc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < C::KS; ++s)
#pragma unroll
          for (int m = 0; m < 4; ++m) dc[m] = vr_mma32<T>(load_wfrag<T>(wf, (mh + m) * C::KS + s, lane), bp[s], dc[m]);
        if (inimg) {
          const size_t pix = (size_t)Y * W + X;
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            HalfT v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = (T)dc[m][i];
            const int kc = 16 * (mh + m) + 4 * q;
            T* const dst = kc < 64 ? dfb + pix * 64 + kc : dff + pix * 64 + kc - 64;
            *reinterpret_cast<HalfT*>(dst) = v;
          }
        }
      }
    }
    __syncthreads();
    // parameter gradients: wave v owns rows 32 v + 16 m + (0..15), m = 0, 1; the contraction runs over the tile's pixels, 32 at a time
#pragma unroll 1
    for (int s = 0; s < C::NPC / 32; ++s) {
      FragT au[2], ad[2];
      int po[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int p = 32 * s + 8 * q + j;
        po[j] = 4 * (p / C::TW) * C::DW + 4 * (p % C::TW);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          au[m][j] = us[p * C::RS + 32 * wave + 16 * m + l16];
          ad[m][j] = dp[p * C::RS + 32 * wave + 16 * m + l16];
        }
      }
#pragma unroll
      for (int eb = 0; eb < C::EB; ++eb) {
        const int ko = koff[16 * eb + l16];
        FragT b;
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] = (T)(ko >= 0 ? dd[ko + po[j]] : 0.f);
#pragma unroll
        for (int m = 0; m < 2; ++m) accl[m][eb] = vr_mma32<T>(au[m], b, accl[m][eb]);
      }
#pragma unroll
      for (int nb = 0; nb < C::MB; ++nb) {
        FragT b;
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] = cs[(32 * s + 8 * q + j) * C::RS + 16 * nb + l16];
#pragma unroll
        for (int m = 0; m < 2; ++m) accf[m][nb] = vr_mma32<T>(ad[m], b, accf[m][nb]);
      }
#pragma unroll
      for (int m = 0; m < 2; ++m) accb[m] = vr_mma32<T>(ad[m], ones, accb[m]);
    }
  }
  float* const slab = parts + (size_t)blockIdx.x * C::SLAB64;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int row = 32 * wave + 16 * m + 4 * q;
#pragma unroll
    for (int eb = 0; eb < C::EB; ++eb)
#pragma unroll
      for (int i = 0; i < 4; ++i) slab[C::S64_WL + (row + i) * 80 + 16 * eb + l16] = accl[m][eb][i];
#pragma unroll
    for (int nb = 0; nb < C::MB; ++nb)
#pragma unroll
      for (int i = 0; i < 4; ++i) slab[C::S64_WFU + (row + i) * 128 + 16 * nb + l16] = accf[m][nb][i];
    if (l16 == 0) {                                        // every column of the ones product holds the same sum
#pragma unroll
      for (int i = 0; i < 4; ++i) slab[C::S64_BFU + row + i] = accb[m][i];
    }
  }
  __syncthreads();
#pragma unroll
  for (int o = 0; o < 3; ++o) dd[o * C::NT + tid] = gsum[o];
  __syncthreads();
  if (tid < 3) {
    float t = 0.f;
    for (int k = 0; k < C::NT; ++k) t += dd[tid * C::NT + k];
    slab[C::S64_BL + tid] = t;
  }
}

// the slabs of mv_recon_bwd64_kernel, summed in workgroup order into dW_fu (2F, 2F) | db_fu (2F) | dW_last (2F, 3, 5, 5) | db_last (3);
// the slab offset of output i is packing.mv_recon_bwd_tables(F)["reduce"][i]: real rows and columns only
__global__ __launch_bounds__(256) void mv_recon_reduce64_kernel(const float* __restrict__ parts, int nslabs, float* __restrict__ grads, int F) {
  typedef MVCfg<float, 64> C;
  const int F2 = 2 * F, n0 = F2 * F2, n1 = n0 + F2, n2 = n1 + F2 * 75, total = n2 + 3;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int off;
  if (i < n0) {
    const int oc = i / F2, ic = i - oc * F2;
    off = C::S64_WFU + oc * 128 + (ic < F ? ic : 64 + ic - F);
  } else if (i < n1) {
    off = C::S64_BFU + (i - n0);
  } else if (i < n2) {
    const int c = (i - n1) / 75, r = (i - n1) - c * 75;
    off = C::S64_WL + c * 80 + r;
  } else {
    off = C::S64_BL + (i - n2);
  }
  float t = 0.f;
  for (int k = 0; k < nslabs; ++k) t += parts[(size_t)k * C::SLAB64 + off];
  grads[i] = t;
}
