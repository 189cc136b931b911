// MATLAB-compatible bicubic downscale of uint8 images on device (gfx950).  Reference op replaced:
// third_party/matlab_imresize/imresize.py:104-136 `imresize(I, scalar_scale=1/scale)` for uint8 input, as
// ImageSuperResolutionBicubicDataset calls it (datasets/_isr.py:170-222): antialiased cubic, two passes, rows (dim 0) first,
// each pass  out = uint8(around(clip(sum_t w[o][t] * in[idx[o][t]], 0, 255)))  with the sum formed in float64, one tap
// after another in tap order (numpy's reduction over a non-innermost axis), and `around` rounding half to even.
// The result is reproduced bit for bit, so:
//   * every product and every sum is a separately rounded double: `#pragma clang fp contract(off)` (hipcc defines
//     __dmul_rn / __dadd_rn as plain `*` / `+` and contracts those into v_fma_f64, which changes the last bit and with it
//     a grey level at a .5 tie);
//   * the weights and the reflected source indices are the host's tables (packing.bicubic_tables): the kernel derives no
//     index of its own.  A tile at the border reads reflected rows / columns, a source shorter than the filter support
//     reflects more than once; whatever the table names is what is read.
//
// One workgroup owns a TH x TW tile of output pixels of one image (or of one training patch):
//   0. its slices of the two tables go to LDS; the smallest and largest source row / column they name bound the window;
//   1. that window of the uint8 source goes to LDS (reflection only folds indices back INTO the span of the unreflected
//      taps, so the window is never larger than (T - 1) * scale + taps + 1 per side: RS x CS below);
//   2. pass 1 (rows): for every output row of the tile and every staged column byte, the double sum -> clip -> rint -> uint8,
//      kept in LDS;
//   3. pass 2 (columns) over that uint8 intermediate, the same way; the caller's `emit` stores the grey level.
// Adjacent threads take adjacent bytes of an LDS row (4 lanes per dword: a broadcast, no bank conflict) and the same
// weight (one broadcast read).
#pragma once
#include "sr_common.h"

namespace bicubic {
constexpr int TH = 16, TW = 32, THREADS = 256;
constexpr int MAX_SCALE = 4;
constexpr int MAXT = 4 * MAX_SCALE + 2;                  // candidate taps of the reference at scale 4 (kept: 16)
constexpr int RS = (TH - 1) * MAX_SCALE + MAXT + 2;      // staged source rows
constexpr int CS = (TW - 1) * MAX_SCALE + MAXT + 2;      // staged source columns
constexpr int ROWB = CS * 3;                             // bytes per staged row (RGB interleaved, as in the image)

struct Smem {
  unsigned char stage[RS * ROWB];
  unsigned char mid[TH * ROWB];
  double wr[TH * MAXT], wc[TW * MAXT];
  int ir[TH * MAXT], ic[TW * MAXT];       // source row / column of every tap, relative to the window after step 0
  int red[4][THREADS / 64];
};

struct Rec { long off; int w, x, y, flags; };            // sr_bicubic_rec_t

SR_DEV double mac(double acc, double w, double p) {
#pragma clang fp contract(off)
  const double m = w * p;
  return acc + m;
}
SR_DEV double mul(double w, double p) {
#pragma clang fp contract(off)
  return w * p;
}
// numpy: around(clip(v, 0, 255)).astype(uint8); rint rounds half to even like around
SR_DEV unsigned char to_u8(double v) { return (unsigned char)(int)rint(fmin(fmax(v, 0.0), 255.0)); }

SR_DEV int wave_min(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m));
  return v;
}
SR_DEV int wave_max(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m));
  return v;
}

// Outputs rows [r0, r0 + nr) x columns [c0, c0 + nc) (nr <= TH, nc <= TW) of the resize of the in_h x in_w view whose pixel
// (0, 0) is at `src`, `stride` pixels per row.  CH_OUTER picks the order in which pass 2 hands results to emit(i, j, ch, v)
// (i, j relative to r0, c0): channel-major for planar outputs, channel-minor for interleaved ones.  Every thread of the
// workgroup must call it.
template <bool CH_OUTER, class Emit>
SR_DEV void tile(Smem& s, const unsigned char* __restrict__ src, long stride, int in_h, int in_w,
                 const double* __restrict__ wr, const int* __restrict__ ir, int tr,
                 const double* __restrict__ wc, const int* __restrict__ ic, int tc,
                 int r0, int nr, int c0, int nc, Emit emit) {
  const int tid = threadIdx.x;
  // 0. table slices; indices are clamped into the view, so a wrong table can give wrong pixels but no stray read
  int rlo = in_h - 1, rhi = 0, clo = in_w - 1, chi = 0;
  for (int e = tid; e < nr * tr; e += THREADS) {
    const int idx = min(max(ir[(long)r0 * tr + e], 0), in_h - 1);
    s.wr[e] = wr[(long)r0 * tr + e];
    s.ir[e] = idx;
    rlo = min(rlo, idx);
    rhi = max(rhi, idx);
  }
  for (int e = tid; e < nc * tc; e += THREADS) {
    const int idx = min(max(ic[(long)c0 * tc + e], 0), in_w - 1);
    s.wc[e] = wc[(long)c0 * tc + e];
    s.ic[e] = idx;
    clo = min(clo, idx);
    chi = max(chi, idx);
  }
  rlo = wave_min(rlo); rhi = wave_max(rhi); clo = wave_min(clo); chi = wave_max(chi);
  if ((tid & 63) == 0) { s.red[0][tid >> 6] = rlo; s.red[1][tid >> 6] = rhi; s.red[2][tid >> 6] = clo; s.red[3][tid >> 6] = chi; }
  __syncthreads();
  rlo = min(min(s.red[0][0], s.red[0][1]), min(s.red[0][2], s.red[0][3]));
  rhi = max(max(s.red[1][0], s.red[1][1]), max(s.red[1][2], s.red[1][3]));
  clo = min(min(s.red[2][0], s.red[2][1]), min(s.red[2][2], s.red[2][3]));
  chi = max(max(s.red[3][0], s.red[3][1]), max(s.red[3][2], s.red[3][3]));
  const int rs = min(rhi - rlo + 1, RS), cb = min(chi - clo + 1, CS) * 3;      // window: rs rows of cb bytes
  for (int e = tid; e < nr * tr; e += THREADS) s.ir[e] = min(s.ir[e] - rlo, RS - 1) * ROWB;
  for (int e = tid; e < nc * tc; e += THREADS) s.ic[e] = min(s.ic[e] - clo, CS - 1) * 3;

  // 1. the window, row by row (rlo + r <= rhi < in_h and clo * 3 + b < (chi + 1) * 3 <= in_w * 3: inside the view)
  for (int e = tid; e < rs * cb; e += THREADS) {
    const int r = e / cb, b = e - r * cb;
    s.stage[r * ROWB + b] = src[((long)(rlo + r) * stride + clo) * 3 + b];
  }
  __syncthreads();

  // 2. rows
  for (int e = tid; e < nr * cb; e += THREADS) {
    const int i = e / cb, b = e - i * cb;
    const double* w = s.wr + i * tr;
    const int* o = s.ir + i * tr;
    double acc = mul(w[0], (double)s.stage[o[0] + b]);
    for (int t = 1; t < tr; ++t) acc = mac(acc, w[t], (double)s.stage[o[t] + b]);
    s.mid[i * ROWB + b] = to_u8(acc);
  }
  __syncthreads();

  // 3. columns
  for (int e = tid; e < nr * nc * 3; e += THREADS) {
    int i, j, ch;
    if constexpr (CH_OUTER) {
      ch = e / (nr * nc);
      const int ij = e - ch * nr * nc;
      i = ij / nc;
      j = ij - i * nc;
    } else {
      i = e / (nc * 3);
      const int jc = e - i * nc * 3;
      j = jc / 3;
      ch = jc - j * 3;
    }
    const double* w = s.wc + j * tc;
    const int* o = s.ic + j * tc;
    const unsigned char* m = s.mid + i * ROWB + ch;
    double acc = mul(w[0], (double)m[o[0]]);
    for (int t = 1; t < tc; ++t) acc = mac(acc, w[t], (double)m[o[t]]);
    emit(i, j, ch, to_u8(acc));
  }
}
}  // namespace bicubic

// grid (tiles_x * tiles_y): out_u8 [Ho][Wo][3] and / or out_f [3][Ho][Wo] = value / 255 (to_tensor); src_f (may be NULL)
// [3][H][W] = the source itself / 255, the HR side of an evaluation item, shared out over the same workgroups
__global__ __launch_bounds__(bicubic::THREADS) void sr_bicubic_resize_kernel(
    const unsigned char* __restrict__ img, unsigned char* __restrict__ out_u8, float* __restrict__ out_f, float* __restrict__ src_f,
    int H, int W, int Ho, int Wo,
    const double* __restrict__ wr, const int* __restrict__ ir, int tr, const double* __restrict__ wc, const int* __restrict__ ic, int tc,
    int tiles_x) {
  using namespace bicubic;
  __shared__ Smem s;
  const int r0 = (int)(blockIdx.x / tiles_x) * TH, c0 = (int)(blockIdx.x % tiles_x) * TW;
  tile<false>(s, img, W, H, W, wr, ir, tr, wc, ic, tc, r0, min(TH, Ho - r0), c0, min(TW, Wo - c0),
              [&](int i, int j, int ch, unsigned char v) {
                const size_t px = (size_t)(r0 + i) * Wo + (c0 + j);
                if (out_u8) out_u8[px * 3 + ch] = v;
                if (out_f) out_f[(size_t)ch * Ho * Wo + px] = (float)v / 255.0f;
              });
  if (src_f) {
    const size_t plane = (size_t)H * W, step = (size_t)gridDim.x * THREADS;
    for (size_t e = (size_t)blockIdx.x * THREADS + threadIdx.x; e < 3 * plane; e += step) {
      const size_t c = e / plane, px = e - c * plane;
      src_f[e] = (float)img[px * 3 + c] / 255.0f;
    }
  }
}

// grid (lr_tiles + hr_blocks, B).  Per record: the HR crop is the S x S square (S = (P + 2 ig) scale) at row x, column y of its
// image; LR patch = the centre P x P of the crop's resize (taps reflect at the CROP's edges: the reference resizes the crop);
// HR patch = the centre (P scale)^2 of the crop; both / 255, then flip rows, flip columns, swap axes as sr_patch_gather_kernel.
__global__ __launch_bounds__(bicubic::THREADS) void sr_bicubic_patch_kernel(
    const unsigned char* __restrict__ cache, const bicubic::Rec* __restrict__ recs, float* __restrict__ lr_out, float* __restrict__ hr_out,
    int P, int scale, int ig, const double* __restrict__ wt, const int* __restrict__ it, int taps, int lr_tiles, int tiles_x) {
  using namespace bicubic;
  __shared__ Smem s;
  const Rec rc = recs[blockIdx.y];
  const int S = (P + 2 * ig) * scale;
  const unsigned char* crop = cache + rc.off + ((size_t)rc.x * rc.w + rc.y) * 3;
  if ((int)blockIdx.x < lr_tiles) {
    const int pr0 = (int)(blockIdx.x / tiles_x) * TH, pc0 = (int)(blockIdx.x % tiles_x) * TW;     // in patch coordinates
    float* o = lr_out + (size_t)blockIdx.y * 3 * P * P;
    tile<true>(s, crop, rc.w, S, S, wt, it, taps, wt, it, taps, ig + pr0, min(TH, P - pr0), ig + pc0, min(TW, P - pc0),
               [&](int i, int j, int ch, unsigned char v) {
                 int r = pr0 + i, q = pc0 + j;
                 if (rc.flags & 1) r = P - 1 - r;
                 if (rc.flags & 2) q = P - 1 - q;
                 const int oi = (rc.flags & 4) ? q : r, oj = (rc.flags & 4) ? r : q;
                 o[((size_t)ch * P + oi) * P + oj] = (float)v / 255.0f;
               });
    return;
  }
  const int HS = P * scale, total = 3 * HS * HS, nblk = gridDim.x - lr_tiles;
  const unsigned char* centre = crop + ((size_t)ig * scale * rc.w + ig * scale) * 3;
  float* o = hr_out + (size_t)blockIdx.y * total;
  for (int e = (blockIdx.x - lr_tiles) * THREADS + threadIdx.x; e < total; e += nblk * THREADS) {
    const int c = e / (HS * HS), ij = e - c * HS * HS, i = ij / HS, j = ij - i * HS;
    int r = (rc.flags & 4) ? j : i, q = (rc.flags & 4) ? i : j;
    if (rc.flags & 1) r = HS - 1 - r;
    if (rc.flags & 2) q = HS - 1 - q;
    o[e] = (float)centre[((size_t)r * rc.w + q) * 3 + c] / 255.0f;
  }
}
