// 7x7 convolutions of SPyNet's BasicModule (gfx950, bf16 MFMA).  Reference op: models/spynet_arch.py:17-22 -- five
// nn.Conv2d(k=7, pad=3) 8 -> 32 -> 64 -> 32 -> 16 -> 2 with ReLU between, run on six pyramid levels (:63-77).  These are the
// one place on the path where the contraction is deep (K = 49 Cin = 392 ... 3136): an implicit GEMM on the matrix cores,
// output channels in rows, 32 pixels of one image row on the lanes, K walked tap by tap.
//
// One workgroup = 8 waves = an 8 x 32 pixel output tile (one row per wave); the (8 + 6) x (32 + 6) input halo tile sits in LDS
// in NHWC order (all Cin channels of a pixel contiguous), so a lane's B fragment of k-step (ky, kx, 16-channel chunk) is ONE
// 16-byte read at a compile-time offset from its pixel.  The weights are packed on the host as MFMA A fragments in exactly the
// order the loop consumes them and streamed through LDS one kernel row at a time by LDS-DMA (<= 28 KB per row, double
// buffered: row ky + 1 lands while row ky is multiplied).  Cin = 8 (first layer) packs two horizontally adjacent taps into
// one 16-deep k-step.  Both operands come from LDS, so the kernel is LDS-bandwidth bound at about half the matrix rate -- the
// register-resident-weights form of wdsr_fwd_rs.h does not apply (a layer's weights are 25 - 200 KB).
//
// TRAINING (SpyNet.hot_training).  Backward-data is the same kernel (BWD): the input gradient of a 7x7 / pad 3 convolution is a
// 7x7 / pad 3 convolution of dy with the weights rotated by 180 degrees and the channel roles swapped, so the transposed layers
// 32 -> 8, 64 -> 32, 32 -> 64, 16 -> 32 and 2 (padded to 8) -> 16 run through the tile scheme above on a second packed table
// (packing.conv7_bwd_tables).  The BWD epilogue has no bias and no ReLU of its own: it multiplies by the ReLU mask of the layer's
// input (a_l > 0, read from the SAVED bf16 activation at the same pixel) and stores dx_l in bf16; the first layer stores its
// 8-channel dx_0 in fp32 without a mask.  The weight gradient (conv7_wgrad_kernel, below) contracts over pixels.
// Rounding points of the backward: the incoming fp32 flow gradient is rounded ONCE to bf16 (by the caller, as it pads it to 8
// channels); every dx_l (l >= 1) is rounded once to bf16 after the mask, and that value is both the next backward-data operand
// and the weight-gradient operand; x_l are the bf16 activations the forward wrote; every accumulation is fp32; db is summed in
// fp32 from the bf16 dy, per workgroup slab and then over the slabs in slab order.
#pragma once
#include "wdsr_fwd_rs.h"

template <int CIN, int COUT> struct Conv7Cfg {
  static_assert(CIN == 8 || CIN % 16 == 0, "input channels: 8 or a multiple of 16");
  static constexpr int TH = 8, TW = 32, HH = TH + 6, HW = TW + 6;
  static constexpr int MT = (COUT + 31) / 32;                      // 32-row output-channel tiles
  static constexpr int KPR = CIN == 8 ? 4 : 7 * (CIN / 16);        // k-steps per kernel row
  static constexpr int FR_ROW = KPR * MT;                          // weight fragments per kernel row
  static constexpr int X_ELEMS = (HH * HW + 2) * CIN;              // (+2 pixels: the paired tap of the last column reads one past)
  static constexpr int LDS_BYTES = X_ELEMS * 2 + 2 * FR_ROW * 1024;
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

// x: [N][H][W][CIN] bf16; w: packed fragments [7][KPR][MT][64 lanes][8]; bias: [MT * 32] fp32 (zero past COUT);
// y: [N][H][W][COUT] bf16 (OUT_F32: fp32).  grid = (tiles_x * tiles_y, N), 512 threads.
// BWD (backward-data: x = dy, w = the rotated, role-swapped table, y = dx): no bias; the bf16 store is multiplied by the mask
// act > 0, act: [N][H][W][COUT] bf16, the saved input of the forward layer; the fp32 store (first layer) takes no mask.
template <int CIN, int COUT, bool RELU, bool OUT_F32, bool BWD = false>
__global__ __launch_bounds__(512) void conv7_fwd_kernel(const __bf16* __restrict__ x, const __bf16* __restrict__ w,
                                                        const float* __restrict__ bias, void* __restrict__ yv, int H, int W,
                                                        int tiles_x, const __bf16* __restrict__ act = nullptr) {
  static_assert(!BWD || !RELU, "backward-data: the mask is the forward's, not a ReLU of the result");
  typedef Conv7Cfg<CIN, COUT> K;
  __shared__ __attribute__((aligned(16))) char smem_raw[K::LDS_BYTES];
  __bf16* const Xs = reinterpret_cast<__bf16*>(smem_raw);
  __bf16* const Ws = Xs + K::X_ELEMS;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = blockIdx.y, tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * K::TH, tx0 = (tile % tiles_x) * K::TW;
  const __bf16* xin = x + (size_t)n * H * W * CIN;

  auto stage_w = [&](int ky) {                          // kernel row ky: FR_ROW fragments of 1 KB, as they lie
    const char* src = reinterpret_cast<const char*>(w) + (size_t)ky * K::FR_ROW * 1024;
    const unsigned dst = lds_addr(Ws) + (ky & 1) * K::FR_ROW * 1024;
#pragma unroll 1
    for (int p = wave; p < K::FR_ROW; p += 8) dma_piece16(src + p * 1024 + lane * 16, dst + p * 1024);
  };
  stage_w(0);
  {                                                     // input halo tile, zero outside the image
    constexpr int CH = CIN / 8, TOTAL = (K::HH * K::HW + 2) * CH;
    for (int idx = tid; idx < TOTAL; idx += 512) {
      const int p = idx / CH, c = idx - p * CH;
      const int py = p / K::HW, px = p - py * K::HW;
      const int Y = ty0 - 3 + py, X = tx0 - 3 + px;
      bf16x8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (__bf16)0.f;
      if (p < K::HH * K::HW && Y >= 0 && Y < H && X >= 0 && X < W) v = *reinterpret_cast<const bf16x8*>(xin + ((size_t)Y * W + X) * CIN + c * 8);
      *reinterpret_cast<bf16x8*>(Xs + idx * 8) = v;
    }
  }
  f32x16 acc[K::MT];
#pragma unroll
  for (int m = 0; m < K::MT; ++m) {                     // bias: row (i & 3) + 8 (i >> 2) + 4 hh of tile m
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[m][i] = BWD ? 0.f : bias[m * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh];
  }
  const __bf16* const xrow = Xs + (wave * K::HW + r) * CIN;       // this lane's pixel at tap (0, 0)
#pragma unroll 1
  for (int ky = 0; ky < 7; ++ky) {
    wait_vmcnt<0>();                                    // this wave's pieces of row ky (and, the first time, nothing else)
    __syncthreads();                                    // ... everybody's; the previous row's reads are over
    if (ky + 1 < 7) stage_w(ky + 1);
    const __bf16* const wl = Ws + (ky & 1) * K::FR_ROW * 512;
    const __bf16* const xk = xrow + ky * K::HW * CIN;
#pragma unroll
    for (int s = 0; s < K::KPR; ++s) {
      // B fragment: Cin >= 16: tap kx = s / (CIN / 16), channels 16 (s % (CIN / 16)) + 8 hh ..; Cin = 8: tap kx = 2 s + hh, all 8
      const int off = CIN == 8 ? (2 * s + hh) * 8 : (s / (CIN / 16)) * CIN + (s % (CIN / 16)) * 16 + hh * 8;
      const bf16x8 b = *reinterpret_cast<const bf16x8*>(xk + off);
#pragma unroll
      for (int m = 0; m < K::MT; ++m)
        acc[m] = mma16<__bf16>(lds_chunk<__bf16>(wl, ((s * K::MT + m) * 64 + lane) * 8), b, acc[m]);
    }
  }
  const int Y = ty0 + wave, X = tx0 + r;
  if (Y < H && X < W) {
    const size_t pix = ((size_t)n * H + Y) * W + X;
#pragma unroll
    for (int m = 0; m < K::MT; ++m) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int ch = m * 32 + g * 8 + hh * 4;         // channels ch .. ch + 3 in regs 4 g .. 4 g + 3
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = RELU ? fmaxf(acc[m][4 * g + k], 0.f) : acc[m][4 * g + k];
        if constexpr (OUT_F32) {
          float* y = reinterpret_cast<float*>(yv) + pix * COUT;
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (ch + k < COUT) y[ch + k] = v[k];
        } else {
          __bf16* y = reinterpret_cast<__bf16*>(yv) + pix * COUT;
          if constexpr (BWD) {
            static_assert(COUT % 8 == 0, "backward-data, bf16 store: whole channel groups");
            const bf16x4 a = *reinterpret_cast<const bf16x4*>(act + pix * COUT + ch);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = (float)a[k] > 0.f ? v[k] : 0.f;
          }
          if (ch + 4 <= COUT) {
            __bf16 o0, o1, o2, o3;
            cvt_pair<__bf16>(o0, o1, v[0], v[1]);
            cvt_pair<__bf16>(o2, o3, v[2], v[3]);
            bf16x4 o;
            o[0] = o0; o[1] = o1; o[2] = o2; o[3] = o3;
            *reinterpret_cast<bf16x4*>(y + ch) = o;
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (ch + k < COUT) y[ch + k] = (__bf16)v[k];
          }
        }
      }
    }
  }
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------------
// dW[co][ci][ky][kx] = sum_{n, y, x} dy[n, y, x, co] x[n, y + ky - 3, x + kx - 3, ci] (zero outside the image), db[co] = sum dy.
// An MFMA product with output channels in rows, (tap, 32 input channels) in columns and PIXELS as K: 32 x 32 accumulator tiles
// (row tile rt, column tile ct, tap), plus one bias tile per row tile (B = ones: every column holds sum dy).  Both operands lie
// NHWC in memory, so K is the strided dimension: a 16 x 16 pixel tile of dy and its 22 x 22 halo tile of x are staged into LDS as
// PLANES of 32 channels ([plane][pixel][32], 64-byte pixel rows) and read back transposed (tr_frag: ds_read_b64_tr_b16, 16
// pixels per k-step).  A 32-lane half reads 4 consecutive pixels x 64 bytes = 256 contiguous bytes, all 64 banks once; a single
// 64-channel image (128-byte rows) would put pixels q and q + 2 on the same banks.  Channels past CA / CB are zero planes' tails.
// No float atomics: workgroup w walks the pixel tiles w, w + wgs, .. in that order and writes its NTL tiles to slab w
// (partial[w][tile][16][64]); unpack_all_kernel (wdsr_prep.h) then sums the slabs in slab order into the flat weight | bias
// gradient through the tables of packing.conv7_wgrad_tables.  Tiles are dealt to (tile group blockIdx.y, wave, j) as in
// rm_wgrad_kernel: 8 waves x 4 accumulators per workgroup.
template <int CA, int CB> struct Conv7WgradCfg {
  static_assert(CA % 8 == 0 && CB % 8 == 0, "whole 16-byte channel groups");
  static constexpr int TW = 16, TH = 16, NPX = TW * TH, KSP = NPX / 16, SW = TW + 6, NPB = SW * (TH + 6);
  static constexpr int NRT = (CA + 31) / 32, NCT = (CB + 31) / 32;
  static constexpr int NCOL = NCT * 49 + 1;                         // per row tile: (column tile, tap) pairs + the bias tile
  static constexpr int NTL = NRT * NCOL, NW = 8, TPW = 4, TPG = NW * TPW, NG = (NTL + TPG - 1) / TPG;
  static constexpr int LDS_BYTES = (NRT * NPX + NCT * NPB) * 32 * 2;
  static constexpr int SLAB = NTL * 1024;                           // floats per workgroup slab
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

// NHWC image (CH channels) -> NPL planes [pixel][32] of an RW-wide pixel window at (y0, x0); zero outside the image and past CH
template <int CH, int NPL, int RW, int NPIX>
SR_DEV void conv7_stage_planes(__bf16* dst, const __bf16* __restrict__ src, int H, int W, int y0, int x0, int tid) {
  constexpr int NC = NPL * 4, TOTAL = NPIX * NC;
  for (int idx = tid; idx < TOTAL; idx += 512) {
    const int p = idx / NC, c = idx - p * NC;
    const int py = p / RW, px = p - py * RW;
    const int Y = y0 + py, X = x0 + px;
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (__bf16)0.f;
    if (c * 8 < CH && Y >= 0 && Y < H && X >= 0 && X < W) v = *reinterpret_cast<const bf16x8*>(src + ((size_t)Y * W + X) * CH + c * 8);
    *reinterpret_cast<bf16x8*>(dst + ((c >> 2) * NPIX + p) * 32 + (c & 3) * 8) = v;
  }
}

// dy: [N][H][W][CA] bf16; xin: [N][H][W][CB] bf16; partial: [gridDim.x][NTL][16][64] fp32.  grid = (wgs, NG), 512 threads.
template <int CA, int CB>
__global__ __launch_bounds__(512) void conv7_wgrad_kernel(const __bf16* __restrict__ dy, const __bf16* __restrict__ xin,
                                                          float* __restrict__ partial, int N, int H, int W, int tiles_x,
                                                          int tiles_per_img) {
  typedef Conv7WgradCfg<CA, CB> C;
  __shared__ __attribute__((aligned(16))) char smem_raw[C::LDS_BYTES];
  __bf16* const GA = reinterpret_cast<__bf16*>(smem_raw);
  __bf16* const XB = GA + C::NRT * C::NPX * 32;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = blockIdx.y;
  const size_t img = (size_t)H * W;
  f32x16 acc[C::TPW];
#pragma unroll
  for (int j = 0; j < C::TPW; ++j) acc[j] = zero16();
  bf16x8 ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = (__bf16)1.f;
  const int total = N * tiles_per_img;
  for (int it = blockIdx.x; it < total; it += gridDim.x) {
    const int n = it / tiles_per_img, ti = it - n * tiles_per_img;
    const int ty = ti / tiles_x, tx = ti - ty * tiles_x;
    const int ty0 = ty * C::TH, tx0 = tx * C::TW;
    __syncthreads();                                               // the previous tile's reads are done
    conv7_stage_planes<CA, C::NRT, C::TW, C::NPX>(GA, dy + n * img * CA, H, W, ty0, tx0, tid);
    conv7_stage_planes<CB, C::NCT, C::SW, C::NPB>(XB, xin + n * img * CB, H, W, ty0 - 3, tx0 - 3, tid);
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < C::KSP; ++s) {
#pragma unroll
      for (int j = 0; j < C::TPW; ++j) {
        const int t = grp * C::TPG + j * C::NW + wave;             // wave-uniform
        if (t < C::NTL) {
          const int rt = t / C::NCOL, col = t - rt * C::NCOL;
          const bf16x8 a = tr_frag<__bf16>(GA + rt * C::NPX * 32, s, lane, [](int p) { return p * 32; });
          bf16x8 b;
          if (col == C::NCT * 49) {
            b = ones;
          } else {
            const int ct = col / 49, tap = col - ct * 49;
            const int ky = tap / 7, kx = tap - ky * 7;
            b = tr_frag<__bf16>(XB + ct * C::NPB * 32, s, lane, [&](int p) { return (((p >> 4) + ky) * C::SW + (p & 15) + kx) * 32; });
          }
          acc[j] = mma16<__bf16>(a, b, acc[j]);
        }
      }
    }
  }
  float* slab = partial + (size_t)blockIdx.x * C::SLAB;
#pragma unroll
  for (int j = 0; j < C::TPW; ++j) {
    const int t = grp * C::TPG + j * C::NW + wave;
    if (t < C::NTL) slab_store_tile(slab, t, acc[j], lane);
  }
}
