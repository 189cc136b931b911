// Parameter plumbing of the video networks' one-call training step (sr_fn_net_train_step, its _sized form at any output size, and
// sr_mf_net_train_step; models/clip_train.py):
// the weight norm of every weight-normed conv and the gather of all trained tensors into the packers' fp32 source vector in ONE launch,
// the index packing of the forward, backward and encoder blobs in one, and -- after the network's own forward and loss-folded backward
// -- the weight-norm backward onto (weight_g, weight_v) with the Adam step of EVERY trained tensor in one.  Reference: the weight norm of
// torch.nn.utils.weight_norm(conv, dim 0) as models/single_image_model.py and models/naive_multi_model_easy.py apply it, and
// train_video_superresolution.py:86-100 (backward, optimizer.step()).
//
// All three take their table BY VALUE in the kernel arguments, as adam_step_multi_kernel (train_step.h) does: optimizer state may be
// re-created by load_state_dict() between two steps, and a table copied to the device per step would cost the launch it saves.  Capacity:
// HIP passes at most 4096 bytes of kernel arguments; a ClipStepRow is 80 bytes (eight pointers, rows, row length, first workgroup), the
// Adam scalars 24, the loss fold 32: CLIP_STEP_CAP = 48 rows = 3904 bytes.  A weight-normed conv is ONE row (g, v and both their states),
// every other tensor (bias, plain conv, ConvTranspose2d) one: Result_Model(4, 32, 8, 3) has 38 rows, Naive_model with 8 blocks 36.
// Workgroup b finds its row by bisection over the uniform table (blk0 ascending from 0), as adam_step_multi_kernel.
//   weight-normed row   one WAVE per output row (the norm runs over len = in kh kw, 27 .. 288): workgroup blk0 + j serves rows 4 j .. 4 j + 3
//   plain row           workgroup blk0 + j serves elements [1024 j, 1024 j + 1024), adam_step_kernel's chunk
// Reductions: lane l sums elements l, l + 64, .. in ascending order, then the xor-shuffle tree 32, 16, .., 1: a fixed order, no atomics.
// Every store is a plain vector-memory store.
#pragma once
#include "sr_common.h"
#include "train_step.h"

constexpr int CLIP_STEP_CAP = 48, CLIP_STEP_CHUNK = 1024, CLIP_PACK_JOBS = 3, CLIP_PACK_CHUNK = 1024;

SR_DEV float clip_wave_sum(float s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  return s;
}

// ---- 1: w = g v / |v| and the gather ------------------------------------------------------------------------------------------------
struct ClipWnRow {
  const float* g;                                       // weight_g (rows); nullptr: a plain row, dst = v
  const float* v;                                       // weight_v (rows x len), or the plain tensor (len elements)
  float* dst;                                           // the effective tensor's place in the source vector
  float* inv;                                           // 1 / |v| per row (weight-normed rows), read again by the backward
  int rows, len, blk0, pad;
};
struct ClipWnTable {
  ClipWnRow row[CLIP_STEP_CAP];
  int count, pad;
};
static_assert(sizeof(ClipWnTable) <= 4096, "the weight-norm table must fit the kernel-argument segment");

template <typename Table>
SR_DEV int clip_find_row(const Table& t) {
  int lo = 0, hi = t.count - 1;                         // the last row with blk0 <= blockIdx.x (uniform: scalar loads of the arguments)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t.row[mid].blk0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void clip_wn_fwd_kernel(const ClipWnTable t) {
  const int r = clip_find_row(t);
  const float* __restrict__ const g = t.row[r].g;
  const float* __restrict__ const v = t.row[r].v;
  float* __restrict__ const dst = t.row[r].dst;
  const int len = t.row[r].len, local = (int)blockIdx.x - t.row[r].blk0;
  if (g == nullptr) {
    const int i0 = local * CLIP_STEP_CHUNK;
    const int i1 = min(i0 + CLIP_STEP_CHUNK, len);
    for (int i = i0 + threadIdx.x; i < i1; i += 256) dst[i] = v[i];
    return;
  }
  const int lane = threadIdx.x & 63, row = local * 4 + (threadIdx.x >> 6);
  if (row >= t.row[r].rows) return;
  const float* const vr = v + (long)row * len;
  float ss = 0.f;
  for (int k = lane; k < len; k += 64) ss = __builtin_fmaf(vr[k], vr[k], ss);
  ss = clip_wave_sum(ss);
  const float inv = 1.0f / __builtin_sqrtf(ss);
  const float s = g[row] * inv;
  for (int k = lane; k < len; k += 64) dst[(long)row * len + k] = vr[k] * s;
  if (lane == 0) t.row[r].inv[row] = inv;
}

// clip_wn_fwd_kernel with the arithmetic of torch._weight_norm(v, g, 0) on the device (sr_fn_net_train_step_sized: its forward has to
// equal the model's own no_grad forward, whose blobs are packed from torch's weight norm, bit for bit in fp32 too).  ATen's kernel gives
// a row one workgroup of CLIP_WN_ATEN_BLOCK threads, thread t accumulates the squares of elements t, t + BLOCK, .. (a fused
// multiply-add each), and the BLOCK values are summed as a tree over strides BLOCK / 2 .. 64 (through LDS), 32 (the first 32 threads),
// then a shuffle-down over 16 .. 1; |v| = sqrt(sum), rnorm = 1 / |v|, w = (g v) rnorm.  Here one wave holds the row, lane l the sums of
// threads l + 64 k, and adds them in that order, every addition rounded on its own.
constexpr int CLIP_WN_ATEN_BLOCK = 256;
__global__ __launch_bounds__(256) void clip_wn_fwd_aten_kernel(const ClipWnTable t) {
  const int r = clip_find_row(t);
  const float* __restrict__ const g = t.row[r].g;
  const float* __restrict__ const v = t.row[r].v;
  float* __restrict__ const dst = t.row[r].dst;
  const int len = t.row[r].len, local = (int)blockIdx.x - t.row[r].blk0;
  if (g == nullptr) {
    const int i0 = local * CLIP_STEP_CHUNK;
    const int i1 = min(i0 + CLIP_STEP_CHUNK, len);
    for (int i = i0 + threadIdx.x; i < i1; i += 256) dst[i] = v[i];
    return;
  }
  const int lane = threadIdx.x & 63, row = local * 4 + (threadIdx.x >> 6);
  if (row >= t.row[r].rows) return;
  const float* const vr = v + (long)row * len;
  constexpr int NK = CLIP_WN_ATEN_BLOCK / 64;
  float a[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    a[k] = 0.f;
    for (int i = lane + 64 * k; i < len; i += CLIP_WN_ATEN_BLOCK) a[k] = __fmaf_rn(vr[i], vr[i], a[k]);
  }
#pragma unroll
  for (int h = NK / 2; h > 0; h >>= 1)                                                                                          // strides BLOCK / 2 .. 64
#pragma unroll
    for (int k = 0; k < h; ++k) a[k] = __fadd_rn(a[k], a[k + h]);
  float f = a[0];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) f = __fadd_rn(f, __shfl_down(f, o));                                                         // 32 .. 1: lane 0 holds the sum
  const float norm = __builtin_sqrtf(__shfl(f, 0));
  const float inv = 1.0f / norm, gr = g[row];
  for (int k = lane; k < len; k += 64) dst[(long)row * len + k] = __fmul_rn(__fmul_rn(gr, vr[k]), inv);
  if (lane == 0) t.row[r].inv[row] = inv;
}

// ---- 2: the index packing: blob[i] = (T) src[idx[i]] for up to three blobs -----------------------------------------------------------
struct ClipPackJob {
  const long* idx;
  void* dst;
  long n;
  int blk0, pad;
};
struct ClipPackTable {
  ClipPackJob row[CLIP_PACK_JOBS];
  int count, pad;
};

template <typename T>
__global__ __launch_bounds__(256) void clip_pack_kernel(const float* __restrict__ src, const ClipPackTable t) {
  const int r = clip_find_row(t);
  const long* __restrict__ const idx = t.row[r].idx;
  T* __restrict__ const dst = (T*)t.row[r].dst;
  const long n = t.row[r].n;
  const long i0 = ((long)((int)blockIdx.x - t.row[r].blk0) * 256 + threadIdx.x) * 4;
  if (i0 + 3 < n) {
    const long a = idx[i0], b = idx[i0 + 1], c = idx[i0 + 2], d = idx[i0 + 3];
    typedef T V __attribute__((ext_vector_type(4)));
    V o;
    o[0] = (T)src[a]; o[1] = (T)src[b]; o[2] = (T)src[c]; o[3] = (T)src[d];
    *reinterpret_cast<V*>(dst + i0) = o;
  } else {
    for (long i = i0; i < n; ++i) dst[i] = (T)src[idx[i]];
  }
}

// ---- 3: the weight-norm backward and Adam ----------------------------------------------------------------------------------------------
// Weight-normed row, per output row with dw = gscale x (its slice of the flat effective-weight gradient), i = 1 / |v| from the forward:
//   s = sum dw v;  dg = s i;  dv = (g i) (dw - v (s i i))
// then adam_elem (train_step.h: adam_step_kernel's arithmetic, instruction for instruction) on g and on every element of v.  Plain row:
// adam_elem on the tensor with gscale x its slice.  The gradient is rounded to fp32 BEFORE it enters Adam (no contraction across the
// two), so the step is the one torch.optim.Adam takes from that gradient, bit for bit.  The last workgroup of the launch that carries
// loss_out also folds the backward's per-workgroup loss sums (loss_sum_kernel's order).
struct ClipStepRow {
  float* p0;                                            // weight_g (rows), or the plain tensor (len elements)
  float* p1;                                            // weight_v (rows x len); nullptr: a plain row
  float* m0;
  float* v0;                                            // exp_avg, exp_avg_sq of p0
  float* m1;
  float* v1;                                            // of p1
  const float* dw;                                      // the tensor's slice of the flat gradient vector
  const float* inv;                                     // clip_wn_fwd_kernel's 1 / |v| per row
  int rows, len, blk0, pad;
};
struct ClipStepTable {
  ClipStepRow row[CLIP_STEP_CAP];
  AdamArgs a;
  float gscale, loss_scale;
  const float* loss_part;
  float* loss_out;                                      // nullptr: this launch does not fold the loss
  int n_loss, count;
};
static_assert(sizeof(ClipStepTable) <= 4096, "the step table must fit the kernel-argument segment");

SR_DEV float clip_keep(float x) {
  asm volatile("" : "+v"(x));                           // x as rounded to fp32 here: nothing contracts across this point
  return x;
}

__global__ __launch_bounds__(256) void clip_wn_bwd_adam_kernel(const ClipStepTable t) {
  const int lane = threadIdx.x & 63;
  if (t.loss_out && blockIdx.x == gridDim.x - 1) {      // the launch has one workgroup more than the rows need
    if (threadIdx.x < 64) {
      float s = 0.f;
      for (int i = lane; i < t.n_loss; i += 64) s += t.loss_part[i];
      s = clip_wave_sum(s);
      if (lane == 0) *t.loss_out = s * t.loss_scale;
    }
    return;
  }
  const int r = clip_find_row(t);
  const AdamArgs a = t.a;
  const float gscale = t.gscale;
  const float* __restrict__ const dw = t.row[r].dw;
  const int len = t.row[r].len, local = (int)blockIdx.x - t.row[r].blk0;
  if (t.row[r].p1 == nullptr) {
    float* __restrict__ const p = t.row[r].p0;
    float* __restrict__ const m = t.row[r].m0;
    float* __restrict__ const v = t.row[r].v0;
    const int i0 = local * CLIP_STEP_CHUNK;
    const int i1 = min(i0 + CLIP_STEP_CHUNK, len);
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
      const float gi = clip_keep(dw[i] * gscale);
      float pi = p[i], mi = m[i], vi = v[i];
      adam_elem(pi, gi, mi, vi, a);
      p[i] = pi; m[i] = mi; v[i] = vi;
    }
    return;
  }
  const int row = local * 4 + (threadIdx.x >> 6);
  if (row >= t.row[r].rows) return;
  const long base = (long)row * len;
  float* __restrict__ const pv = t.row[r].p1 + base;
  float* __restrict__ const mv = t.row[r].m1 + base;
  float* __restrict__ const vv = t.row[r].v1 + base;
  const float* __restrict__ const dwr = dw + base;
  float s = 0.f;
  for (int k = lane; k < len; k += 64) s = __builtin_fmaf(clip_keep(dwr[k] * gscale), pv[k], s);
  s = clip_wave_sum(s);
  const float inv = t.row[r].inv[row], g = t.row[r].p0[row];
  const float dg = clip_keep(s * inv);
  const float gi = g * inv, proj = dg * inv;            // g / |v|, s / |v|^2
  for (int k = lane; k < len; k += 64) {
    float pk = pv[k], mk = mv[k], vk = vv[k];
    const float gk = clip_keep(gi * (clip_keep(dwr[k] * gscale) - pk * proj));
    adam_elem(pk, gk, mk, vk, a);
    pv[k] = pk; mv[k] = mk; vv[k] = vk;
  }
  if (lane == 0) {
    float pg = g, mg = t.row[r].m0[row], vg = t.row[r].v0[row];
    adam_elem(pg, dg, mg, vg, a);
    t.row[r].p0[row] = pg; t.row[r].m0[row] = mg; t.row[r].v0[row] = vg;
  }
}
