// Video training clips cut on device from a resident frame cache (gfx950).  Reference ops replaced, per clip item (TRAIN mode,
// train_sample_patch): VideoSuperResolutionDataset / VideoSuperResolutionWithMVHdf5Dataset `__getitem__` -- `_sample_patch`
// (the same crop at LR row x, column y for every frame; HR at scale times that; MV the LR window), `to_tensor` (HWC uint8 ->
// CHW float32 / 255; MV: permute only, already float32 in the cache), the stack over frames and `_augment` (p1 < 0.5: reverse
// the width, p2 < 0.5: reverse the height, on every frame) -- datasets/_vsr.py:59-180, :314-432.  The draws stay on the
// host in the reference's own RNG order; one 24-byte record per clip tells the kernel what to cut.
//
// One lane cuts a run of RUN pixels along one output row: one wide load of the run's 3 RUN source bytes (the dword-aligned
// 16 bytes around them), the horizontal flip done in registers (the run is read from the mirrored source position and
// reversed), one dwordx4 store per channel plane.  The vertical flip only moves the source row.  A row whose length is not a
// multiple of RUN ends in a shorter run cut pixel by pixel.  The aligned 16 bytes may reach 3 bytes past a run's last byte: the
// cache ends in 16 bytes of padding (datasets.DeviceClipCache).
#pragma once
#include "sr_common.h"

struct ClipRec { long ids_off; int x, y, flags, T; };                  // flags: 1 reverse the width, 2 reverse the height
struct ClipFrame { long lr_off, hr_off, mv_off; int lr_w, hr_w; };     // byte offsets (cache / mv cache), widths in pixels

namespace clips {

constexpr int RUN = 4;   // pixels per lane

typedef float f32x4 __attribute__((ext_vector_type(4)));

// RUN floats at o: one dwordx4 store when `vec` (o 16-byte aligned: every run of a row whose length is a multiple of RUN,
// the launcher checks the bases), else dword stores
__device__ __forceinline__ void store_run(float* o, const float (&v)[RUN], bool vec) {
  if (vec) {
    *(f32x4*)o = f32x4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int m = 0; m < RUN; ++m) o[m] = v[m];
  }
}

// n pixels of HWC uint8 at src -> planes o, o + plane, o + 2 plane (float32 / 255), pixel m of the output = source pixel
// (hf ? n - 1 - m : m)
__device__ __forceinline__ void cut_rgb(const unsigned char* src, float* o, size_t plane, int n, bool hf, bool vec) {
  if (n == RUN) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4), aligned(4)));
    const unsigned lo = (unsigned)(uintptr_t)src & 3u, sh = lo * 8;
    const u32x4 d = *(const u32x4*)(src - lo);
    const unsigned w[3] = {(unsigned)((((unsigned long long)d.y << 32) | d.x) >> sh),
                           (unsigned)((((unsigned long long)d.z << 32) | d.y) >> sh),
                           (unsigned)((((unsigned long long)d.w << 32) | d.z) >> sh)};
    float f[3][RUN], v[3][RUN];
#pragma unroll
    for (int m = 0; m < RUN; ++m) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int k = 3 * m + c;
        f[c][m] = (float)((w[k >> 2] >> (8 * (k & 3))) & 255u) / 255.0f;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int m = 0; m < RUN; ++m) v[c][m] = hf ? f[c][RUN - 1 - m] : f[c][m];
      store_run(o + c * plane, v[c], vec);
    }
  } else {
    for (int m = 0; m < n; ++m) {
      const int sm = hf ? n - 1 - m : m;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c * plane + m] = (float)src[3 * sm + c] / 255.0f;
    }
  }
}

// n pixels of HW2 float32 at src (8-byte aligned) -> planes o, o + plane
__device__ __forceinline__ void cut_mv(const float* src, float* o, size_t plane, int n, bool hf, bool vec) {
  if (n == RUN) {
    float2 p[RUN];
    float v0[RUN], v1[RUN];
#pragma unroll
    for (int m = 0; m < RUN; ++m) p[m] = *(const float2*)(src + 2 * m);
#pragma unroll
    for (int m = 0; m < RUN; ++m) {
      v0[m] = hf ? p[RUN - 1 - m].x : p[m].x;
      v1[m] = hf ? p[RUN - 1 - m].y : p[m].y;
    }
    store_run(o, v0, vec);
    store_run(o + plane, v1, vec);
  } else {
    for (int m = 0; m < n; ++m) {
      const int sm = hf ? n - 1 - m : m;
      o[m] = src[2 * sm];
      o[plane + m] = src[2 * sm + 1];
    }
  }
}

}  // namespace clips

// grid (ceil(items / 256) capped, B * T); items of one frame: P rows x ceil(P / RUN) runs of LR (+ MV), then S rows x
// ceil(S / RUN) runs of HR, S = P * scale.  lr_out [B][T][C][P][P] with C = 3, or 5 when mv_cache is given (channels 3, 4 =
// the motion vector); hr_out [B][T][3][S][S]; either may be NULL.
__global__ __launch_bounds__(256) void sr_clip_gather_kernel(const unsigned char* __restrict__ cache, const float* __restrict__ mv_cache,
                                                             const ClipFrame* __restrict__ frames, const int* __restrict__ ids,
                                                             const ClipRec* __restrict__ recs, float* __restrict__ lr_out,
                                                             float* __restrict__ hr_out, int T, int P, int scale) {
  using clips::RUN;
  const int bt = blockIdx.y, b = bt / T, t = bt - b * T;
  const ClipRec rc = recs[b];
  if (t >= rc.T) return;                                   // (never with the records DeviceClipCache writes: T is every clip's length)
  const ClipFrame fr = frames[ids[rc.ids_off + t]];
  const int S = P * scale, RL = (P + RUN - 1) / RUN, RH = (S + RUN - 1) / RUN;
  const int nL = lr_out ? P * RL : 0, nH = hr_out ? S * RH : 0;
  const int C = mv_cache ? 5 : 3;
  const bool hf = rc.flags & 1, vf = rc.flags & 2, vl = (P & (RUN - 1)) == 0, vh = (S & (RUN - 1)) == 0;
  const size_t pl = (size_t)P * P, ph = (size_t)S * S;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < nL + nH; e += gridDim.x * 256) {
    if (e < nL) {
      const int i = e / RL, j0 = (e - i * RL) * RUN, n = min(RUN, P - j0);
      const long r = rc.x + (vf ? P - 1 - i : i), s0 = rc.y + (hf ? P - j0 - n : j0);
      float* o = lr_out + (size_t)bt * C * pl + (size_t)i * P + j0;
      clips::cut_rgb(cache + fr.lr_off + (r * fr.lr_w + s0) * 3, o, pl, n, hf, vl);
      if (mv_cache)
        clips::cut_mv((const float*)((const unsigned char*)mv_cache + fr.mv_off) + (r * fr.lr_w + s0) * 2, o + 3 * pl, pl, n, hf, vl);
    } else {
      const int eh = e - nL, i = eh / RH, j0 = (eh - i * RH) * RUN, n = min(RUN, S - j0);
      const long r = (long)rc.x * scale + (vf ? S - 1 - i : i), s0 = (long)rc.y * scale + (hf ? S - j0 - n : j0);
      clips::cut_rgb(cache + fr.hr_off + (r * fr.hr_w + s0) * 3, hr_out + (size_t)bt * 3 * ph + (size_t)i * S + j0, ph, n, hf, vh);
    }
  }
}
