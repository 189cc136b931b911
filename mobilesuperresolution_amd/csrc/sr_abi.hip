// C-ABI entry points of libsr_hotpath.so (declared in include/sr_hotpath.h).
#include <algorithm>
#include <cmath>
#include "../../include/sr_hotpath.h"
#include "wdsr_block.h"
#include "wdsr_fwd_rs.h"
#include "wdsr_fwd_stream.h"
#include "wdsr_bwd_rs.h"
#include "wdsr_bwd_pair_lds.h"
#include "wdsr_wgrad_rs.h"
#include "wdsr_ends.h"
#include "wdsr_prep.h"
#include "conv3x3.h"
#include "conv64.h"
#include "conv64_bwd.h"
#include "vsr_recon.h"
#include "vsr_recon_bwd.h"
#include "mv_recon.h"
#include "spynet_conv.h"
#include "nas_block.h"
#include "nas_dw_lc.h"
#include "nas_bwd_fused.h"
#include "flow_warp.h"
#include "metrics.h"
#include "ssim.h"
#include "eval.h"
#include "patches.h"
#include "clips.h"
#include "bicubic.h"
#include "train_step.h"
#include "pixel_shuffle.h"
#include "result_block.h"
#include "frame_net.h"
#include "frame_net_bwd.h"
#include "multi_frame.h"
#include "multi_frame_bwd.h"
#include "clip_param_step.h"

extern "C" int sr_abi_version(void) { return 25; }

namespace {

// The block geometry of each supported width, written once: F units expand to E channels and contract to L.  The kernels keep
// their <F, E, L> parameters; the host code names a width and reads the rest here.
template <int F_, int E_, int L_>
struct WdsrDimsOf {
  static constexpr int F = F_, E = E_, L = L_;
  typedef BlockCfg<F_, E_, L_> Cfg;
};
template <int F> struct WdsrDims;
template <> struct WdsrDims<24> : WdsrDimsOf<24, 144, 20> {};
template <> struct WdsrDims<32> : WdsrDimsOf<32, 192, 26> {};

// runtime width -> fn(WdsrDims<F>{}), for a generic lambda that reads F off its argument's type; -1 for a width without kernels
template <typename Fn>
int dispatch_f(int F, Fn&& fn) {
  if (F == 24) return fn(WdsrDims<24>{});
  if (F == 32) return fn(WdsrDims<32>{});
  return -1;
}
// runtime (width, dtype) -> fn(WdsrDims<F>{}, T{})
template <typename Fn>
int dispatch_ft(int F, int dtype, Fn&& fn) {
  return dispatch_f(F, [&](auto d) {
    if (dtype == SR_DTYPE_BF16) return fn(d, __bf16{});
    if (dtype == SR_DTYPE_F32) return fn(d, float{});
    return -1;
  });
}

// workgroup tiles over an H x W image (the spatial tile is the same at every width)
struct Tiles { int x, y; };
template <typename C = WdsrDims<24>::Cfg>
Tiles block_tiles(int H, int W) {
  return Tiles{(W + C::TW - 1) / C::TW, (H + C::TH - 1) / C::TH};
}

template <typename T, int F>
int launch_block_fwd(const void* x, void* y, const void* wblob, const float* cinit, int N, int H, int W,
                     hipStream_t st, void* tsave = nullptr) {
  typedef typename WdsrDims<F>::Cfg C;
  const auto [tiles_x, tiles_y] = block_tiles<C>(H, W);
  dim3 grid(tiles_x * tiles_y, N), block(64 * C::NPT_H);
  hipLaunchKernelGGL((wdsr_block_fwd_kernel<T, F, C::E, C::L>), grid, block, 0, st, (const T*)x, (T*)y, (const T*)wblob,
                     cinit, H, W, tiles_x, (T*)tsave);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

template <typename T, int F>
int launch_block_bwd_data(const void* x, const void* dy, void* dx, const void* wblob, const float* cinit, int N,
                          int H, int W, hipStream_t st, void* dtsave = nullptr) {
  typedef typename WdsrDims<F>::Cfg C;
  const auto [tiles_x, tiles_y] = block_tiles<C>(H, W);
  dim3 grid(tiles_x * tiles_y, N), block(64 * C::NPT_O);
  hipLaunchKernelGGL((wdsr_block_bwd_data_kernel<T, F, C::E, C::L>), grid, block, 0, st, (const T*)x, (const T*)dy, (T*)dx,
                     (const T*)wblob, cinit, H, W, tiles_x, (T*)dtsave);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

template <typename T, int F>
int launch_block_wgrad(const void* x, const void* dy, const void* wblob, const float* cinit, float* pa, float* pb,
                       int layers, int wgs, int N, int H, int W, long x_ls, long dy_ls, long w_ls, long c_ls,
                       hipStream_t st) {
  typedef typename WdsrDims<F>::Cfg C;
  const auto [tiles_x, tiles_y] = block_tiles<C>(H, W);
  dim3 grid(wgs, layers);
  hipLaunchKernelGGL((wdsr_block_wgrad_kernel<T, F, C::E, C::L, 0>), grid, dim3(64 * WgradCfg<F, C::E, C::L, 0>::NWAVES), 0, st,
                     (const T*)x, (const T*)dy, (const T*)wblob, cinit, pa, N, H, W, tiles_x, tiles_x * tiles_y, x_ls,
                     dy_ls, w_ls, c_ls);
  hipLaunchKernelGGL((wdsr_block_wgrad_kernel<T, F, C::E, C::L, 1>), grid, dim3(64 * WgradCfg<F, C::E, C::L, 1>::NWAVES), 0, st,
                     (const T*)x, (const T*)dy, (const T*)wblob, cinit, pb, N, H, W, tiles_x, tiles_x * tiles_y, x_ls,
                     dy_ls, w_ls, c_ls);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// one image per workgroup pays from one image per CU on, when the last round of workgroups is at least ~70 % full
static bool fwd_stream_applies(long N, int H, int W) {
  if (W != 48 || H % 4 != 0 || H < 8 || H > 4096 || N < 256) return false;
  const long rounds = (N + 255) / 256;
  return N * 10 >= rounds * 256 * 7;
}

// the sixteen-wave form (weights read from LDS at use): the forward of the 32-unit network, whose weight sets do not fit the
// register-resident kernels
template <int F, int NBLK>
static int launch_fwd_rs16(const void* x, void* ya, void* yb, const void* wa, const void* wb, const float* cia, const float* cib,
                           void* tsa, void* tsb, int N, int H, int W, hipStream_t st) {
  typedef typename WdsrDims<F>::Cfg C;
  typedef __bf16 T;
  constexpr int E = C::E, L = C::L;
  const auto [tiles_x, tiles_y] = block_tiles<C>(H, W);
  if (tsa && (NBLK == 1 || tsb))
    hipLaunchKernelGGL((wdsr_fwd_rs16_kernel<F, E, L, NBLK, true>), dim3(tiles_x * tiles_y, N), dim3(1024), 0, st, (const T*)x, (T*)ya,
                       (T*)yb, (const T*)wa, (const T*)wb, cia, cib, (T*)tsa, (T*)tsb, H, W, tiles_x);
  else
    hipLaunchKernelGGL((wdsr_fwd_rs16_kernel<F, E, L, NBLK, false>), dim3(tiles_x * tiles_y, N), dim3(1024), 0, st, (const T*)x, (T*)ya,
                       (T*)yb, (const T*)wa, (const T*)wb, cia, cib, (T*)tsa, (T*)tsb, H, W, tiles_x);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

// forward with register-resident weights (csrc/wdsr_fwd_rs.h): nblk = 1 (x -> yb) or 2 (x -> ya -> yb)
template <int F, int NBLK>
static int launch_fwd_rs(const void* x, void* ya, void* yb, const void* wa, const void* wb, const float* cia, const float* cib,
                         void* tsa, void* tsb, int N, int H, int W, hipStream_t st) {
  typedef typename WdsrDims<F>::Cfg C;
  typedef __bf16 T;
  constexpr int E = C::E, L = C::L;
  const auto [tiles_x, tiles_y] = block_tiles<C>(H, W);
  constexpr int persist_from = 768;                    // measured crossover: 3 tiles per CU
  const long total = (long)N * tiles_x * tiles_y;
  if constexpr (NBLK == 2) {
    // whole 48-wide images, at least one per CU and the last round of workgroups reasonably full: the streaming kernel
    // (csrc/wdsr_fwd_stream.h: no halo recompute, one barrier per band), with or without the saved t images
    if (fwd_stream_applies(N, H, W)) {
      if (tsa && tsb)
        hipLaunchKernelGGL((wdsr_fwd_stream12_kernel<F, E, L, true>), dim3(256), dim3(768), 0, st, (const T*)x, (T*)ya, (T*)yb, (const T*)wa,
                           (const T*)wb, cia, cib, (T*)tsa, (T*)tsb, N, H);
      else
        hipLaunchKernelGGL((wdsr_fwd_stream12_kernel<F, E, L, false>), dim3(256), dim3(768), 0, st, (const T*)x, (T*)ya, (T*)yb, (const T*)wa,
                           (const T*)wb, cia, cib, (T*)nullptr, (T*)nullptr, N, H);
      SR_HIP_CHECK_LAUNCH();
      return 0;
    }
  }
  if (total >= persist_from && total < (1L << 31)) {   // many tiles per CU: the persistent form (one workgroup per CU)
    const int wgs = 256;
    const bool save = tsa && (NBLK == 1 || tsb);
    if (save && NBLK == 1) {
      hipLaunchKernelGGL((wdsr_fwd_rs_persist_kernel<F, E, L, 1, true>), dim3(wgs), dim3(512), 0, st, (const T*)x, (T*)ya, (T*)yb,
                         (const T*)wa, (const T*)wb, cia, cib, (T*)tsa, (T*)tsb, N, H, W, tiles_x, tiles_x * tiles_y);
      SR_HIP_CHECK_LAUNCH();
      return 0;
    }
    if constexpr (NBLK == 2) {
      if (!save) {                                     // two blocks, nothing saved: the two-role pipeline
        hipLaunchKernelGGL((wdsr_fwd_rs_pipe_kernel<F, E, L>), dim3(wgs), dim3(512), 0, st, (const T*)x, (T*)ya, (T*)yb, (const T*)wa,
                           (const T*)wb, cia, cib, N, H, W, tiles_x, tiles_x * tiles_y);
        SR_HIP_CHECK_LAUNCH();
        return 0;
      }
    } else if (!save) {
      hipLaunchKernelGGL((wdsr_fwd_rs_persist_kernel<F, E, L, 1, false>), dim3(wgs), dim3(512), 0, st, (const T*)x, (T*)ya, (T*)yb,
                         (const T*)wa, (const T*)wb, cia, cib, (T*)tsa, (T*)tsb, N, H, W, tiles_x, tiles_x * tiles_y);
      SR_HIP_CHECK_LAUNCH();
      return 0;
    }
  }
  if (tsa && (NBLK == 1 || tsb))
    hipLaunchKernelGGL((wdsr_fwd_rs_kernel<F, E, L, NBLK, true>), dim3(tiles_x * tiles_y, N), dim3(512), 0, st, (const T*)x, (T*)ya,
                       (T*)yb, (const T*)wa, (const T*)wb, cia, cib, (T*)tsa, (T*)tsb, H, W, tiles_x);
  else
    hipLaunchKernelGGL((wdsr_fwd_rs_kernel<F, E, L, NBLK, false>), dim3(tiles_x * tiles_y, N), dim3(512), 0, st, (const T*)x, (T*)ya,
                       (T*)yb, (const T*)wa, (const T*)wb, cia, cib, (T*)tsa, (T*)tsb, H, W, tiles_x);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
// 24 units: the eight-wave kernels; 32 units: the sixteen-wave form
template <int F, int NBLK>
static int launch_fwd_rs_any(const void* x, void* ya, void* yb, const void* wa, const void* wb, const float* cia, const float* cib,
                             void* tsa, void* tsb, int N, int H, int W, hipStream_t st) {
  if constexpr (F == 24) return launch_fwd_rs<F, NBLK>(x, ya, yb, wa, wb, cia, cib, tsa, tsb, N, H, W, st);
  else return launch_fwd_rs16<F, NBLK>(x, ya, yb, wa, wb, cia, cib, tsa, tsb, N, H, W, st);
}
extern "C" int sr_wdsr_fwd_rs(const void* x, void* ya, void* yb, const void* wa, const void* wb, const float* cia,
                              const float* cib, void* tsa, void* tsb, int nblk, int N, int H, int W, int F, int dtype,
                              sr_stream_t stream) {
  if (!x || !yb || !wa || !cia || N <= 0 || H <= 0 || W <= 0 || N > 65535 || (nblk == 2 && (!wb || !cib))) return -2;
  if (dtype != SR_DTYPE_BF16) return -1;
  hipStream_t st = (hipStream_t)stream;
  return dispatch_f(F, [&](auto d) {
    if (nblk == 2) return launch_fwd_rs_any<decltype(d)::F, 2>(x, ya, yb, wa, wb, cia, cib, tsa, tsb, N, H, W, st);
    if (nblk == 1) return launch_fwd_rs_any<decltype(d)::F, 1>(x, nullptr, yb, wa, nullptr, cia, nullptr, tsa, nullptr, N, H, W, st);
    return -1;
  });
}
extern "C" int sr_wdsr_block2_fwd(const void* x, void* ya, void* yb, const void* wa, const void* wb, const float* cia,
                                  const float* cib, void* tsa, void* tsb, int N, int H, int W, int F, int dtype,
                                  sr_stream_t stream) {
  if (F != 24 && F != 32) return (!x || !yb || !wa || !wb || !cia || !cib || N <= 0 || H <= 0 || W <= 0 || N > 65535) ? -2 : -1;
  return sr_wdsr_fwd_rs(x, ya, yb, wa, wb, cia, cib, tsa, tsb, 2, N, H, W, F, dtype, stream);
}
extern "C" int sr_wdsr_fwd_rs_repeat(void* x, void* ya, void* yb, const void* wa, const void* wb, const float* cia,
                                     const float* cib, void* tsa, void* tsb, int nblk, int N, int H, int W, int F, int dtype,
                                     int reps, sr_stream_t stream) {
  for (int i = 0; i < reps; ++i) {
    const int rc = (i & 1) ? sr_wdsr_fwd_rs(yb, ya, x, wa, wb, cia, cib, tsa, tsb, nblk, N, H, W, F, dtype, stream)
                           : sr_wdsr_fwd_rs(x, ya, yb, wa, wb, cia, cib, tsa, tsb, nblk, N, H, W, F, dtype, stream);
    if (rc) return rc;
  }
  return 0;
}

extern "C" int sr_wdsr_block_fwd_repeat(void* x, void* y, const void* wblob, const float* cinit, int N, int H, int W,
                                        int F, int dtype, int reps, sr_stream_t stream) {
  for (int i = 0; i < reps; ++i) {
    const int rc = (i & 1) ? sr_wdsr_block_fwd(y, x, wblob, cinit, N, H, W, F, dtype, stream)
                           : sr_wdsr_block_fwd(x, y, wblob, cinit, N, H, W, F, dtype, stream);
    if (rc) return rc;
  }
  return 0;
}

extern "C" int sr_wdsr_block2_fwd_repeat(void* x, void* ya, void* yb, const void* wa, const void* wb, const float* cia,
                                         const float* cib, int N, int H, int W, int F, int dtype, int reps,
                                         sr_stream_t stream) {
  for (int i = 0; i < reps; ++i) {
    const int rc = (i & 1) ? sr_wdsr_block2_fwd(yb, ya, x, wa, wb, cia, cib, nullptr, nullptr, N, H, W, F, dtype, stream)
                           : sr_wdsr_block2_fwd(x, ya, yb, wa, wb, cia, cib, nullptr, nullptr, N, H, W, F, dtype, stream);
    if (rc) return rc;
  }
  return 0;
}

extern "C" int sr_wdsr_block_bwd_data(const void* x, const void* dy, void* dx, const void* wblob,
                                      const float* cinit, int N, int H, int W, int F, int dtype,
                                      sr_stream_t stream) {
  if (!x || !dy || !dx || !wblob || !cinit || N <= 0 || H <= 0 || W <= 0 || N > 65535) return -2;
  return dispatch_ft(F, dtype, [&](auto d, auto t) {
    return launch_block_bwd_data<decltype(t), decltype(d)::F>(x, dy, dx, wblob, cinit, N, H, W, (hipStream_t)stream);
  });
}

extern "C" int sr_wdsr_block2_bwd_data(const void* xa, const void* xb, const void* dyb, void* dxb, void* dxa,
                                       const void* wa, const void* wb, const float* cia, const float* cib, void* dta,
                                       void* dtb, int N, int H, int W, int F, int dtype, sr_stream_t stream) {
  if (!xa || !xb || !dyb || !dxb || !dxa || !wa || !wb || !cia || !cib || N <= 0 || H <= 0 || W <= 0 || N > 65535)
    return -2;
  if ((F != 24 && F != 32) || dtype != SR_DTYPE_BF16) return -1;
  const auto [tiles_x, tiles_y] = block_tiles(H, W);
  if (F == 32) {                                       // 32 units: twelve waves, fragments from LDS at use (csrc/wdsr_bwd_pair_lds.h)
    typedef WdsrDims<32> D;
    hipLaunchKernelGGL((wdsr_bwd_pair_lds_kernel<32, D::E, D::L>), dim3(tiles_x * tiles_y, N), dim3(BwdPairCfg<32, D::E, D::L>::NTHREADS),
                       0, (hipStream_t)stream, (const __bf16*)xa, (const __bf16*)xb, (const __bf16*)dyb, (__bf16*)dxb, (__bf16*)dxa,
                       (const __bf16*)wa, (const __bf16*)wb, cia, cib, (__bf16*)dta, (__bf16*)dtb, H, W, tiles_x);
  } else {                                             // 24 units: eight waves, register-resident weights (csrc/wdsr_bwd_rs.h)
    typedef WdsrDims<24> D;
    hipLaunchKernelGGL((wdsr_bwd_rs_kernel<24, D::E, D::L>), dim3(tiles_x * tiles_y, N), dim3(512), 0, (hipStream_t)stream,
                       (const __bf16*)xa, (const __bf16*)xb, (const __bf16*)dyb, (__bf16*)dxb, (__bf16*)dxa, (const __bf16*)wa,
                       (const __bf16*)wb, (__bf16*)dta, (__bf16*)dtb, H, W, tiles_x);
  }
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

extern "C" int sr_wdsr_block_wgrad(const void* x, const void* dy, const void* wblob, const float* cinit,
                                   float* pa, float* pb, int layers, int wgs, int N, int H, int W, int F,
                                   int dtype, long x_ls, long dy_ls, long w_ls, long c_ls, sr_stream_t stream) {
  if (!x || !dy || !wblob || !cinit || !pa || !pb || layers <= 0 || wgs <= 0 || N <= 0 || H <= 0 || W <= 0 ||
      layers > 65535)
    return -2;
  return dispatch_ft(F, dtype, [&](auto d, auto t) {
    return launch_block_wgrad<decltype(t), decltype(d)::F>(x, dy, wblob, cinit, pa, pb, layers, wgs, N, H, W, x_ls, dy_ls, w_ls, c_ls,
                                                           (hipStream_t)stream);
  });
}

namespace {
template <int F>
int launch_wgrad_saved(const void* x, const void* dy, const void* tsave, const void* dtsave, const void* wblob,
                       const float* cinit, float* pa, float* pb, int layers, int wgs, int N, int H, int W, long x_ls,
                       long dy_ls, long side_ls, long w_ls, long c_ls, hipStream_t st) {
  typedef typename WdsrDims<F>::Cfg C;
  typedef __bf16 T;
  constexpr int E = C::E, L = C::L;
  const auto [tiles_x, tiles_y] = block_tiles<C>(H, W);
  dim3 grid(wgs, layers);
  const bool old_a = (long)N * tiles_x * tiles_y * C::TH * C::TW >= (1L << 31);   // (the 8-wave kernel indexes pixels in 32 bits)
  if constexpr (F == 24) {
    if (!old_a)
      hipLaunchKernelGGL((wdsr_wgrad_a8_kernel<F, E, L>), grid, dim3(WgradA8Cfg<F, E, L>::NTHREADS), 0, st, (const T*)x, (const T*)dtsave,
                         (const T*)wblob, pa, N, H, W, tiles_x, tiles_x * tiles_y, x_ls, side_ls, w_ls);
  }
  if (F != 24 || old_a)
    hipLaunchKernelGGL((wdsr_block_wgrad_saved_kernel<T, F, E, L, 0>), grid, dim3(64 * WgradSavedCfg<F, E, L>::NWAVES), 0, st,
                       (const T*)x, (const T*)dtsave, (const T*)wblob, cinit, pa, N, H, W, tiles_x, tiles_x * tiles_y, x_ls,
                       side_ls, w_ls, c_ls);
  hipLaunchKernelGGL((wdsr_wgrad_b8_kernel<F, E, L>), grid, dim3(WgradB8Cfg<F, E, L>::NTHREADS), 0, st, (const T*)dy, (const T*)tsave,
                     pb, N, H, W, tiles_x, tiles_x * tiles_y, dy_ls, side_ls);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
}  // namespace

extern "C" int sr_wdsr_block_wgrad_saved(const void* x, const void* dy, const void* tsave, const void* dtsave,
                                         const void* wblob, const float* cinit, float* pa, float* pb, int layers, int wgs,
                                         int N, int H, int W, int F, int dtype, long x_ls, long dy_ls, long side_ls,
                                         long w_ls, long c_ls, sr_stream_t stream) {
  if (!x || !dy || !tsave || !dtsave || !wblob || !cinit || !pa || !pb || layers <= 0 || wgs <= 0 || N <= 0 || H <= 0 ||
      W <= 0 || layers > 65535)
    return -2;
  if (dtype != SR_DTYPE_BF16) return -1;
  return dispatch_f(F, [&](auto d) {
    return launch_wgrad_saved<decltype(d)::F>(x, dy, tsave, dtsave, wblob, cinit, pa, pb, layers, wgs, N, H, W, x_ls, dy_ls, side_ls,
                                                  w_ls, c_ls, (hipStream_t)stream);
  });
}

extern "C" int sr_wdsr_block_slab_sizes(int F, int* slab_a, int* slab_b) {
  if (!slab_a || !slab_b) return -2;
  return dispatch_f(F, [&](auto d) {
    typedef BwdCfg<typename decltype(d)::Cfg> B;
    *slab_a = B::SLAB_A;
    *slab_b = B::SLAB_B;
    return 0;
  });
}

extern "C" int sr_wdsr_block_fwd(const void* x, void* y, const void* wblob, const float* cinit, int N, int H,
                                 int W, int F, int dtype, sr_stream_t stream) {
  if (!x || !y || !wblob || !cinit || N <= 0 || H <= 0 || W <= 0 || N > 65535) return -2;
  return dispatch_ft(F, dtype, [&](auto d, auto t) {
    return launch_block_fwd<decltype(t), decltype(d)::F>(x, y, wblob, cinit, N, H, W, (hipStream_t)stream);
  });
}

// ------------------------------------------------------------------------------------------
// head / tail
// ------------------------------------------------------------------------------------------
namespace {
template <typename E> dim3 tile_grid(int N, int H, int W, int* tiles_x) {
  *tiles_x = (W + E::TW - 1) / E::TW;
  return dim3(*tiles_x * ((H + E::TH - 1) / E::TH), N);
}
#define SR_DISPATCH_TF(CALL)                                                     \
  if (F == 24 && dtype == SR_DTYPE_BF16) { CALL(__bf16, 24) }                    \
  else if (F == 24 && dtype == SR_DTYPE_F32) { CALL(float, 24) }                 \
  else if (F == 32 && dtype == SR_DTYPE_BF16) { CALL(__bf16, 32) }               \
  else if (F == 32 && dtype == SR_DTYPE_F32) { CALL(float, 32) }                 \
  else return -1;
#define SR_DISPATCH_R(CALL, T, F_)                                               \
  if (R == 4) { CALL(T, F_, 4) } else if (R == 2) { CALL(T, F_, 2) } else if (R == 3) { CALL(T, F_, 3) } else return -1;
}  // namespace

extern "C" int sr_head_fwd(const float* x, void* y, const void* wblob, float mean, int N, int H, int W, int F,
                           int dtype, sr_stream_t stream) {
  if (!x || !y || !wblob || N <= 0 || H <= 0 || W <= 0 || N > 65535) return -2;
  hipStream_t st = (hipStream_t)stream;
#define CALL(T, F_) { typedef EndsCfg<F_, 4> E; int tx; dim3 g = tile_grid<E>(N, H, W, &tx); \
    hipLaunchKernelGGL((sr_head_fwd_kernel<T, F_>), g, dim3(256), 0, st, x, (T*)y, (const T*)wblob, mean, H, W, tx); }
  SR_DISPATCH_TF(CALL)
#undef CALL
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

extern "C" int sr_tail_fwd(const void* feat, const float* x, float* out, const void* wblob, float mean, int N,
                           int H, int W, int F, int R, int dtype, sr_stream_t stream) {
  if (!feat || !x || !out || !wblob || N <= 0 || H <= 0 || W <= 0 || N > 65535) return -2;
  hipStream_t st = (hipStream_t)stream;
#define CALLR(T, F_, R_) { typedef EndsCfg<F_, R_> E; int tx; dim3 g = tile_grid<E>(N, H, W, &tx); \
    hipLaunchKernelGGL((sr_tail_fwd_kernel<T, F_, R_>), g, dim3(SR_TAIL_FWD_THREADS), 0, st, (const T*)feat, x, out, (const T*)wblob, mean, H, W, tx); }
#define CALL(T, F_) SR_DISPATCH_R(CALLR, T, F_)
  SR_DISPATCH_TF(CALL)
#undef CALL
#undef CALLR
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

namespace {
// LOSS = 0: `dout` is d(loss)/d(out).  LOSS = 1 (L1) / 2 (Charbonnier): `dout` is the network output, `hr` the target,
// gscale = upstream gradient / numel; the wgrad / fused kernels also write one loss partial sum per workgroup.
template <int LOSS>
int tail_bwd_data_t(const float* dout, const float* hr, float gscale, void* dfeat, const void* wblob, int N, int H, int W, int F,
                    int R, int dtype, hipStream_t st) {
  const LossIn li{hr, gscale};
#define CALLR(T, F_, R_) { typedef EndsCfg<F_, R_> E; int tx; dim3 g = tile_grid<E>(N, H, W, &tx); \
    hipLaunchKernelGGL((sr_tail_bwd_data_kernel<T, F_, R_, LOSS>), g, dim3(256), 0, st, dout, (T*)dfeat, (const T*)wblob, H, W, tx, li); }
#define CALL(T, F_) SR_DISPATCH_R(CALLR, T, F_)
  SR_DISPATCH_TF(CALL)
#undef CALL
#undef CALLR
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
template <int LOSS>
int tail_wgrad_t(const float* dout, const float* hr, float gscale, float* loss_part, const void* feat, const float* x, float mean,
                 float* partial, int wgs, int N, int H, int W, int F, int R, int dtype, hipStream_t st) {
  const LossIn li{hr, gscale};
#define CALLR(T, F_, R_) { typedef EndsCfg<F_, R_> E; const int tx = (W + E::TW - 1) / E::TW, tpi = tx * ((H + E::TH - 1) / E::TH); \
    hipLaunchKernelGGL((sr_tail_wgrad_kernel<T, F_, R_, LOSS>), dim3(wgs), dim3(896), 0, st, dout, (const T*)feat, x, mean, partial, N, H, W, tx, tpi, li, loss_part); }
#define CALL(T, F_) SR_DISPATCH_R(CALLR, T, F_)
  SR_DISPATCH_TF(CALL)
#undef CALL
#undef CALLR
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
template <int LOSS>
int tail_bwd_t(const float* dout, const float* hr, float gscale, float* loss_part, const void* feat, const float* x, float mean,
               const void* wblob, void* dfeat, float* partial, int wgs, int N, int H, int W, int F, int R, hipStream_t st) {
  const LossIn li{hr, gscale};
  typedef __bf16 TB;
#define CALLR(T, F_, R_) { typedef EndsCfg<F_, R_> E; const int tx = (W + E::TW - 1) / E::TW, tpi = tx * ((H + E::TH - 1) / E::TH); \
    hipLaunchKernelGGL((sr_tail_bwd_kernel<T, F_, R_, LOSS>), dim3(wgs), dim3(896), 0, st, dout, (const T*)feat, x, mean, (const T*)wblob, (T*)dfeat, partial, N, H, W, tx, tpi, li, loss_part); }
  if (F == 24) { SR_DISPATCH_R(CALLR, TB, 24) } else if (F == 32) { SR_DISPATCH_R(CALLR, TB, 32) } else return -1;
#undef CALLR
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
}  // namespace

extern "C" int sr_tail_bwd_data(const float* dout, void* dfeat, const void* wblob, int N, int H, int W, int F,
                                int R, int dtype, sr_stream_t stream) {
  if (!dout || !dfeat || !wblob || N <= 0 || H <= 0 || W <= 0 || N > 65535) return -2;
  return tail_bwd_data_t<0>(dout, nullptr, 0.f, dfeat, wblob, N, H, W, F, R, dtype, (hipStream_t)stream);
}

extern "C" int sr_tail_wgrad(const float* dout, const void* feat, const float* x, float mean, float* partial,
                             int wgs, int N, int H, int W, int F, int R, int dtype, sr_stream_t stream) {
  if (!dout || !feat || !x || !partial || wgs <= 0 || N <= 0 || H <= 0 || W <= 0) return -2;
  return tail_wgrad_t<0>(dout, nullptr, 0.f, nullptr, feat, x, mean, partial, wgs, N, H, W, F, R, dtype, (hipStream_t)stream);
}

extern "C" int sr_tail_bwd(const float* dout, const void* feat, const float* x, float mean, const void* wblob,
                          void* dfeat, float* partial, int wgs, int N, int H, int W, int F, int R, int dtype,
                          sr_stream_t stream) {
  if (!dout || !feat || !x || !wblob || !dfeat || !partial || wgs <= 0 || N <= 0 || H <= 0 || W <= 0) return -2;
  if (dtype != SR_DTYPE_BF16) return -1;
  return tail_bwd_t<0>(dout, nullptr, 0.f, nullptr, feat, x, mean, wblob, dfeat, partial, wgs, N, H, W, F, R, (hipStream_t)stream);
}

// tail backward with the loss folded in: `sr` = network output, `hr` = target (both NCHW fp32 HR), loss_kind 1 = L1,
// 2 = Charbonnier; writes dfeat, the weight-gradient slabs and loss_part[wgs] (sums of |sr - hr| resp. sqrt(d^2 + eps))
extern "C" int sr_tail_bwd_loss(const float* sr, const float* hr, int loss_kind, float gscale, float* loss_part, const void* feat,
                                const float* x, float mean, const void* wblob, void* dfeat, float* partial, int wgs, int N,
                                int H, int W, int F, int R, int dtype, sr_stream_t stream) {
  if (!sr || !hr || !loss_part || !feat || !x || !wblob || !dfeat || !partial || wgs <= 0 || N <= 0 || H <= 0 || W <= 0 || N > 65535)
    return -2;
  if (loss_kind != 1 && loss_kind != 2) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SR_DTYPE_BF16)
    return loss_kind == 1 ? tail_bwd_t<1>(sr, hr, gscale, loss_part, feat, x, mean, wblob, dfeat, partial, wgs, N, H, W, F, R, st)
                          : tail_bwd_t<2>(sr, hr, gscale, loss_part, feat, x, mean, wblob, dfeat, partial, wgs, N, H, W, F, R, st);
  int rc = loss_kind == 1 ? tail_bwd_data_t<1>(sr, hr, gscale, dfeat, wblob, N, H, W, F, R, dtype, st)
                          : tail_bwd_data_t<2>(sr, hr, gscale, dfeat, wblob, N, H, W, F, R, dtype, st);
  if (rc) return rc;
  return loss_kind == 1 ? tail_wgrad_t<1>(sr, hr, gscale, loss_part, feat, x, mean, partial, wgs, N, H, W, F, R, dtype, st)
                        : tail_wgrad_t<2>(sr, hr, gscale, loss_part, feat, x, mean, partial, wgs, N, H, W, F, R, dtype, st);
}

// tail forward + loss + tail backward in one launch (csrc/wdsr_ends.h sr_tail_train_kernel): what sr_tail_fwd followed by
// sr_tail_bwd_loss writes to dfeat, the slabs and loss_part, bit for bit, without the SR image.  bf16, R = 4, F = 24 / 32; -1 otherwise.
extern "C" int sr_tail_train(const float* hr, int loss_kind, float gscale, float* loss_part, const void* feat, const float* x,
                             float mean, const void* wblob, void* dfeat, float* partial, int wgs, int N, int H, int W, int F,
                             int R, int dtype, sr_stream_t stream) {
  if (!hr || !loss_part || !feat || !x || !wblob || !dfeat || !partial || wgs <= 0 || N <= 0 || H <= 0 || W <= 0 || N > 65535)
    return -2;
  if (dtype != SR_DTYPE_BF16 || R != 4 || (F != 24 && F != 32) || (loss_kind != 1 && loss_kind != 2)) return -1;
  hipStream_t st = (hipStream_t)stream;
  const LossIn li{hr, gscale};
  typedef __bf16 TB;
  // every workgroup with at most one tile (the training step at batch <= 32 of 48 x 48): the instantiation without the tile loop
#define LAUNCH(F_, LOSS, ONE) hipLaunchKernelGGL((sr_tail_train_kernel<TB, F_, 4, LOSS, ONE>), dim3(wgs), dim3(896), 0, st, (const TB*)feat, x, mean, (const TB*)wblob, (TB*)dfeat, partial, N, H, W, tx, tpi, li, loss_part)
#define CALL(F_, LOSS) { typedef EndsCfg<F_, 4> E; const int tx = (W + E::TW - 1) / E::TW, tpi = tx * ((H + E::TH - 1) / E::TH); \
    if ((long)wgs >= (long)N * tpi) LAUNCH(F_, LOSS, true); else LAUNCH(F_, LOSS, false); }
  if (F == 24) { if (loss_kind == 1) CALL(24, 1) else CALL(24, 2) }
  else { if (loss_kind == 1) CALL(32, 1) else CALL(32, 2) }
#undef CALL
#undef LAUNCH
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

extern "C" int sr_head_wgrad(const void* dy0, const float* x, float mean, float* partial, int wgs, int N, int H,
                             int W, int F, int dtype, sr_stream_t stream) {
  if (!dy0 || !x || !partial || wgs <= 0 || N <= 0 || H <= 0 || W <= 0) return -2;
  hipStream_t st = (hipStream_t)stream;
#define CALL(T, F_) { typedef EndsCfg<F_, 4> E; const int tx = (W + E::TW - 1) / E::TW, tpi = tx * ((H + E::TH - 1) / E::TH); \
    hipLaunchKernelGGL((sr_head_wgrad_kernel<T, F_>), dim3(wgs), dim3(576), 0, st, (const T*)dy0, x, mean, partial, N, H, W, tx, tpi); }
  SR_DISPATCH_TF(CALL)
#undef CALL
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------
// BasicVSR trunk convolutions
// ------------------------------------------------------------------------------------------
namespace {
struct C3Grid { int tx, tpi; dim3 grid; };
inline C3Grid c3_grid(int N, int H, int W) {
  C3Grid g;
  g.tx = (W + C3Cfg::TW - 1) / C3Cfg::TW;
  g.tpi = g.tx * ((H + C3Cfg::TH - 1) / C3Cfg::TH);
  g.grid = dim3(g.tpi, N);
  return g;
}
template <typename T> C3WarpSrc<T> c3_warp_src(const sr_c3_warp_t* w) {
  C3WarpSrc<T> s{};
  if (w) { s.frame = w->frame; s.state = (const T*)w->state; s.flow = w->flow; s.frame_bs = w->frame_bs; s.flow_bs = w->flow_bs; s.x0_save = (T*)w->x0_save; }
  return s;
}
template <typename T>
int c3_fwd_t(const void* x, const void* res, void* y, const void* w, int N, int H, int W, int CI, int act, hipStream_t st,
             const sr_c3_warp_t* warp = nullptr, C3Dir dir = C3Dir{0, 0}) {
  const C3Grid g = c3_grid(N, H, W);
  const dim3 blk(64 * C3Cfg::NPT_O);
  const C3WarpSrc<T> ws = c3_warp_src<T>(warp);
#define L(CI_, ONES_, ACT_, ADD_) hipLaunchKernelGGL((c3_fwd_kernel<T, CI_, ONES_, ACT_, ADD_>), g.grid, blk, 0, st, (const T*)x, (const T*)res, (T*)y, (const T*)w, H, W, g.tx, ws, dir)
  if (warp) {
    if (CI != 32 || act != 2 || res) return -1;
    hipLaunchKernelGGL((c3_fwd_kernel<T, 32, 27, 2, false, true>), g.grid, blk, 0, st, (const T*)nullptr, (const T*)nullptr, (T*)y,
                       (const T*)w, H, W, g.tx, ws, dir);
  } else if (CI == 32 && act == 2 && !res) L(32, 27, 2, false);
  else if (CI == 24 && act == 2 && !res) L(24, 24, 2, false);      // first conv of ConvResidualBlocks(F, F, n): no frame channels
  else if (CI == 24 && act == 1 && !res) L(24, 24, 1, false);
  else if (CI == 24 && act == 0 && res) L(24, 24, 0, true);
  else if (CI == 24 && act == 0 && !res) L(24, 24, 0, false);
  else return -1;
#undef L
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
template <typename T>
int c3_bwd_t(const void* dA, const void* A, const void* add, void* dx, const void* w, int N, int H, int W, int CI, int act,
             hipStream_t st, C3Dir dir = C3Dir{0, 0}) {
  const C3Grid g = c3_grid(N, H, W);
  const dim3 blk(64 * C3Cfg::NPT_O);
#define L(CI_, ACT_, ADD_) hipLaunchKernelGGL((c3_bwd_data_kernel<T, CI_, ACT_, ADD_>), g.grid, blk, 0, st, (const T*)dA, (const T*)A, (const T*)add, (T*)dx, (const T*)w, H, W, g.tx, dir)
  if (CI == 32 && act == 2 && !add) L(32, 2, false);
  else if (CI == 24 && act == 2 && !add) L(24, 2, false);
  else if (CI == 24 && act == 1 && add) L(24, 1, true);
  else if (CI == 24 && act == 1 && !add) L(24, 1, false);
  else if (CI == 24 && act == 0 && !add) L(24, 0, false);
  else return -1;
#undef L
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
template <typename T>
int c3_wgrad_t(const void* x, const void* dA, const void* A, float* partial, int wgs, int N, int H, int W, int CI, int act,
               hipStream_t st, int layers = 1, long x_ls = 0, long d_ls = 0, long a_ls = 0, long p_ls = 0,
               const sr_c3_warp_t* warp = nullptr, int n_dir = 0) {
  const C3Grid g = c3_grid(N, H, W);
  const C3WarpSrc<T> ws = c3_warp_src<T>(warp);
#define L(CI_, ONES_, ACT_) hipLaunchKernelGGL((c3_wgrad_kernel<T, CI_, ONES_, ACT_>), dim3(wgs, layers), dim3(576), 0, st, (const T*)x, (const T*)dA, (const T*)A, partial, N, H, W, g.tx, g.tpi, x_ls, d_ls, a_ls, p_ls, ws, n_dir)
  if (warp) {
    if (CI != 32 || act != 2 || layers != 1) return -1;
    hipLaunchKernelGGL((c3_wgrad_kernel<T, 32, 27, 2, true>), dim3(wgs, 1), dim3(576), 0, st, (const T*)nullptr, (const T*)dA,
                       (const T*)A, partial, N, H, W, g.tx, g.tpi, x_ls, d_ls, a_ls, p_ls, ws, n_dir);
  } else if (CI == 32 && act == 2) L(32, 27, 2);
  else if (CI == 24 && act == 2) L(24, 24, 2);
  else if (CI == 24 && act == 1) L(24, 24, 1);
  else if (CI == 24 && act == 0) L(24, 24, 0);
  else return -1;
#undef L
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
}  // namespace

extern "C" int sr_c3_fwd(const void* x, const void* res, void* y, const void* wblob, int N, int H, int W, int CI,
                         int act, int dtype, sr_stream_t stream) {
  if (!x || !y || !wblob || N <= 0 || H <= 0 || W <= 0 || N > 65535) return -2;
  return dtype == SR_DTYPE_BF16 ? c3_fwd_t<__bf16>(x, res, y, wblob, N, H, W, CI, act, (hipStream_t)stream)
                                : c3_fwd_t<float>(x, res, y, wblob, N, H, W, CI, act, (hipStream_t)stream);
}
extern "C" int sr_c3_bwd_data(const void* dA, const void* A, const void* add, void* dx, const void* wblob, int N,
                              int H, int W, int CI, int act, int dtype, sr_stream_t stream) {
  if (!dA || !dx || !wblob || (act != 0 && !A) || N <= 0 || H <= 0 || W <= 0 || N > 65535) return -2;
  if (!A) A = dA;
  return dtype == SR_DTYPE_BF16 ? c3_bwd_t<__bf16>(dA, A, add, dx, wblob, N, H, W, CI, act, (hipStream_t)stream)
                                : c3_bwd_t<float>(dA, A, add, dx, wblob, N, H, W, CI, act, (hipStream_t)stream);
}
extern "C" int sr_c3_wgrad(const void* x, const void* dA, const void* A, float* partial, int wgs, int N, int H,
                           int W, int CI, int act, int dtype, sr_stream_t stream) {
  if (!x || !dA || !partial || (act != 0 && !A) || wgs <= 0 || N <= 0 || H <= 0 || W <= 0) return -2;
  if (!A) A = dA;
  return dtype == SR_DTYPE_BF16 ? c3_wgrad_t<__bf16>(x, dA, A, partial, wgs, N, H, W, CI, act, (hipStream_t)stream)
                                : c3_wgrad_t<float>(x, dA, A, partial, wgs, N, H, W, CI, act, (hipStream_t)stream);
}

// whole propagation trunk (ConvResidualBlocks.forward, models/basicvsr_arch.py:108-147) from one call
template <typename T>
static int c3_trunk_fwd_t(const void* x0, const sr_c3_warp_t* warp, void* acts_, void* mids_, const void* blob_,
                          const long* boff, int nb, int N, int H, int W, int ci0, hipStream_t st, C3Dir dir) {
  const size_t act = (size_t)N * H * W * 24;
  T* acts = (T*)acts_; T* mids = (T*)mids_; const T* blob = (const T*)blob_;
  int rc;
  if ((rc = c3_fwd_t<T>(x0, nullptr, acts, blob + boff[0], N, H, W, ci0, 2, st, warp, dir))) return rc;
  for (int i = 0; i < nb; ++i) {
    if constexpr (sizeof(T) == 2) {
      const C3Grid g = c3_grid(N, H, W);
      if (i + 1 < nb) {                                // two residual blocks per launch (odd counts: the last one alone)
        hipLaunchKernelGGL((c3_resblock2_fwd_kernel<T>), g.grid, dim3(64 * C3Quad::NWAVES), 0, st, acts + i * act, mids + i * act,
                           acts + (i + 1) * act, mids + (i + 1) * act, acts + (i + 2) * act, blob, boff[1 + 2 * i], boff[2 + 2 * i],
                           boff[3 + 2 * i], boff[4 + 2 * i], H, W, g.tx, dir);
        SR_HIP_CHECK_LAUNCH();
        ++i;
        continue;
      }
      hipLaunchKernelGGL((c3_resblock_fwd_kernel<T>), g.grid, dim3(64 * C3Pair::NPT_H), 0, st, acts + i * act, mids + i * act,
                         acts + (i + 1) * act, blob + boff[1 + 2 * i], blob + boff[2 + 2 * i], H, W, g.tx, dir);
      SR_HIP_CHECK_LAUNCH();
      continue;
    }
    if ((rc = c3_fwd_t<T>(acts + i * act, nullptr, mids + i * act, blob + boff[1 + 2 * i], N, H, W, 24, 1, st, nullptr, dir))) return rc;
    if ((rc = c3_fwd_t<T>(mids + i * act, acts + i * act, acts + (i + 1) * act, blob + boff[2 + 2 * i], N, H, W, 24, 0, st, nullptr, dir)))
      return rc;
  }
  return 0;
}
template <typename T>
static int c3_trunk_bwd_t(const void* x0, const sr_c3_warp_t* warp, const void* acts_, const void* mids_, void* ga_, void* gt_,
                          const void* blob_, const long* boff, float* parts, void* dx0, const sr_c3_unpack_t* up, int nb,
                          int wgs, int N, int H, int W, int ci0, hipStream_t st, C3Dir dir) {
  const size_t act = (size_t)N * H * W * 24;
  const T* acts = (const T*)acts_; const T* mids = (const T*)mids_; const T* blob = (const T*)blob_;
  T* ga = (T*)ga_; T* gt = (T*)gt_;
  const long slot = (long)wgs * 9 * 1024;
  int rc;
  for (int i = nb - 1; i >= 0; --i) {                // a_{i+1} = a_i + conv2(t_i), t_i = relu(conv1(a_i))
    if constexpr (sizeof(T) == 2) {
      const C3Grid g = c3_grid(N, H, W);
      hipLaunchKernelGGL((c3_resblock_bwd_data_kernel<T>), g.grid, dim3(64 * C3Pair::NPT_H), 0, st, ga + (i + 1) * act,
                         mids + i * act, gt + i * act, ga + i * act, blob + boff[1 + 2 * i], blob + boff[2 + 2 * i], H, W, g.tx, dir);
      SR_HIP_CHECK_LAUNCH();
      continue;
    }
    if ((rc = c3_bwd_t<T>(ga + (i + 1) * act, ga + (i + 1) * act, nullptr, gt + i * act, blob + boff[2 + 2 * i], N, H, W, 24, 0, st, dir)))
      return rc;
    if ((rc = c3_bwd_t<T>(gt + i * act, mids + i * act, ga + (i + 1) * act, ga + i * act, blob + boff[1 + 2 * i], N, H, W, 24, 1, st, dir)))
      return rc;
  }
  if (nb > 0) {                                      // every conv2, then every conv1, one launch each
    if ((rc = c3_wgrad_t<T>(mids, ga + act, ga + act, parts + 2 * slot, wgs, N, H, W, 24, 0, st, nb, (long)act, (long)act,
                            (long)act, 2 * slot, nullptr, dir.n_dir)))
      return rc;
    if ((rc = c3_wgrad_t<T>(acts, gt, mids, parts + slot, wgs, N, H, W, 24, 1, st, nb, (long)act, (long)act, (long)act, 2 * slot,
                            nullptr, dir.n_dir)))
      return rc;
  }
  const bool regather = warp && !warp->x0_save;      // the forward kept the gathered input unless told not to
  if ((rc = c3_wgrad_t<T>(warp && !regather ? warp->x0_save : x0, ga, acts, parts, wgs, N, H, W, ci0, 2, st, 1, 0, 0, 0, 0, regather ? warp : nullptr,
                          dir.n_dir)))
    return rc;
  if (dx0 && (rc = c3_bwd_t<T>(ga, acts, nullptr, dx0, blob + boff[0], N, H, W, ci0, 2, st, dir))) return rc;
  if (warp && (warp->dstate || warp->dflow)) {       // flow_warp backward, gather form (no float atomics)
    if (!dx0 || !warp->dstate || (warp->flow && !warp->flow_bound)) return -2;
    const int tx = (W + C3WarpBwd::TS - 1) / C3WarpBwd::TS, ty = (H + C3WarpBwd::TS - 1) / C3WarpBwd::TS;
    hipLaunchKernelGGL((c3_warp_bwd_kernel<T>), dim3(tx * ty, N), dim3(256), 0, st, (const T*)dx0, c3_warp_src<T>(warp),
                       warp->flow_bound, (T*)warp->dstate, warp->dflow, warp->dflow_bs, H, W, tx);
    SR_HIP_CHECK_LAUNCH();
  }
  if (up) {                                          // slabs -> gradient of the flat parameter (of each trunk: its half of the slabs)
    UnpackSegs us;
    const long slab = 9 * 1024;
    const int ndir = dir.n_dir > 0 ? 2 : 1, wd = wgs / ndir;
    const long total = (long)up->n0 + (nb > 0 ? 2L * nb * up->n1 : 0);
    us.nseg = 0;
    int blk = 0;
    for (int d = 0; d < ndir; ++d) {
      us.s[us.nseg++] = UnpackSeg{parts + (size_t)d * wd * slab, up->sidx0, up->dst0, d * total, 0, slab, wd, up->n0, 1, blk, wgs};
      blk += unpack_blocks(up->n0, wd);
      if (nb > 0) {
        // layer l's slabs start at parts + (1 + l) wgs slab: the stride between layers stays wgs slabs, this trunk's start d wd slabs in
        us.s[us.nseg++] = UnpackSeg{parts + (size_t)wgs * slab + (size_t)d * wd * slab, up->sidx1, up->dst1, d * total + (long)up->n0,
                                    (long)up->n1, slab, wd, up->n1, 2 * nb, blk, wgs};
        blk += 2 * nb * unpack_blocks(up->n1, wd);
      }
    }
    hipLaunchKernelGGL(unpack_all_kernel, dim3(blk), dim3(64 * UNPACK_Q), 0, st, up->gflat, us);
    SR_HIP_CHECK_LAUNCH();
  }
  return 0;
}
extern "C" int sr_c3_trunk_fwd(const void* x0, const sr_c3_warp_t* warp, void* acts, void* mids, const void* blob,
                               const long* blob_off, int nb, int N, int H, int W, int ci0, int dtype, int n_dir, long blob_dir_stride,
                               sr_stream_t stream) {
  if ((!x0) == (!warp) || !acts || (nb > 0 && !mids) || !blob || !blob_off || nb < 0 || N <= 0 || H <= 0 || W <= 0 || N > 65535) return -2;
  if (warp && (!warp->frame || ci0 != 32 || (warp->flow && !warp->state))) return -2;
  if (n_dir < 0 || n_dir >= N) return -2;
  const C3Dir dir{blob_dir_stride, n_dir};
  return dtype == SR_DTYPE_BF16 ? c3_trunk_fwd_t<__bf16>(x0, warp, acts, mids, blob, blob_off, nb, N, H, W, ci0, (hipStream_t)stream, dir)
                                : c3_trunk_fwd_t<float>(x0, warp, acts, mids, blob, blob_off, nb, N, H, W, ci0, (hipStream_t)stream, dir);
}
extern "C" int sr_c3_trunk_bwd(const void* x0, const sr_c3_warp_t* warp, const void* acts, const void* mids, void* ga, void* gt,
                               const void* blob, const long* blob_off, float* parts, void* dx0, const sr_c3_unpack_t* unpack,
                               int nb, int wgs, int N, int H, int W, int ci0, int dtype, int n_dir, long blob_dir_stride,
                               sr_stream_t stream) {
  if ((!x0) == (!warp) || !acts || !ga || (nb > 0 && (!mids || !gt)) || !blob || !blob_off || !parts || nb < 0 || wgs <= 0 || N <= 0 ||
      H <= 0 || W <= 0 || N > 65535)
    return -2;
  if (warp && (!warp->frame || ci0 != 32 || (warp->flow && !warp->state))) return -2;
  if (unpack && (!unpack->sidx0 || !unpack->dst0 || !unpack->gflat || unpack->n0 <= 0 ||
                 (nb > 0 && (!unpack->sidx1 || !unpack->dst1 || unpack->n1 <= 0))))
    return -2;
  if (n_dir < 0 || n_dir >= N || (n_dir > 0 && (wgs & 1))) return -2;
  const C3Dir dir{blob_dir_stride, n_dir};
  return dtype == SR_DTYPE_BF16
             ? c3_trunk_bwd_t<__bf16>(x0, warp, acts, mids, ga, gt, blob, blob_off, parts, dx0, unpack, nb, wgs, N, H, W, ci0, (hipStream_t)stream, dir)
             : c3_trunk_bwd_t<float>(x0, warp, acts, mids, ga, gt, blob, blob_off, parts, dx0, unpack, nb, wgs, N, H, W, ci0, (hipStream_t)stream, dir);
}

// ------------------------------------------------------------------------------------------
// 64-feature propagation trunk, inference (csrc/conv64.h)
// ------------------------------------------------------------------------------------------
namespace {
template <typename T>
int c64_conv_t(const void* x, const void* res, void* y, const void* w, int N, int H, int W, int CI, int act, hipStream_t st,
               const sr_c3_warp_t* warp, C3Dir dir, const void* mask = nullptr, int dz = 0) {
  const C3Grid g = c3_grid(N, H, W);                 // 16 x 16 tiles, as C3Cfg
  const dim3 blk(C64Cfg::NTHREADS);
  C64WarpSrc<T> ws{};
  if (warp) {
    ws.frame = warp->frame; ws.state = (const T*)warp->state; ws.flow = warp->flow; ws.frame_bs = warp->frame_bs; ws.flow_bs = warp->flow_bs;
    ws.x0_save = (T*)warp->x0_save;
  }
#define LK(CI_, ACT_, ADD_, WARP_, DZ_, SAVE_) hipLaunchKernelGGL((c64_conv_kernel<T, CI_, ACT_, ADD_, WARP_, DZ_, SAVE_>), g.grid, blk, 0, st, (const T*)x, (const T*)res, (T*)y, (const T*)w, H, W, g.tx, ws, dir, (const T*)mask)
#define L(CI_, ACT_, ADD_, WARP_) LK(CI_, ACT_, ADD_, WARP_, 0, false)
  if (dz) {                                          // backward-data: conv of the transposed weights on g * act'(mask)
    if (warp || CI != 64 || act != 0 || !mask) return -1;
    if (dz == 1 && res) LK(64, 0, true, false, 1, false);
    else if (dz == 2 && !res) LK(64, 0, false, false, 2, false);
    else return -1;
  } else if (warp) {
    if (CI != 80 || act != 2 || res) return -1;
    if (warp->x0_save) LK(80, 2, false, true, 0, true);
    else L(80, 2, false, true);
  } else if (CI == 64 && act == 0 && !res) L(64, 0, false, false);
  else if (CI == 80 && act == 2 && !res) L(80, 2, false, false);
  else if (CI == 64 && act == 2 && !res) L(64, 2, false, false);
  else if (CI == 64 && act == 1 && !res) L(64, 1, false, false);
  else if (CI == 64 && act == 0 && res) L(64, 0, true, false);
  else return -1;
#undef L
#undef LK
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

// conv0 -> (ping | out); then per block: bf16 one fused launch cur -> the other image of the pair (the last block -> out);
// fp32 conv1 cur -> the other image (t), conv2 + cur -> cur in place (the last block -> out)
template <typename T>
int c64_trunk_fwd_t(const void* x0, const sr_c3_warp_t* warp, void* ping, void* pong, void* out, const void* blob_,
                    const long* boff, int nb, int N, int H, int W, int ci0, hipStream_t st, C3Dir dir) {
  const T* blob = (const T*)blob_;
  T* cur = nb > 0 ? (T*)ping : (T*)out;
  int rc;
  if ((rc = c64_conv_t<T>(x0, nullptr, cur, blob + boff[0], N, H, W, ci0, 2, st, warp, dir))) return rc;
  for (int i = 0; i < nb; ++i) {
    T* other = cur == (T*)ping ? (T*)pong : (T*)ping;
    T* dst = i + 1 == nb ? (T*)out : nullptr;
    if constexpr (sizeof(T) == 2) {
      if (!dst) dst = other;
      const C3Grid g = c3_grid(N, H, W);
      hipLaunchKernelGGL((c64_resblock_kernel<T>), g.grid, dim3(C64Cfg::NTHREADS), 0, st, (const T*)cur, dst, blob + boff[1 + 2 * i],
                         blob + boff[2 + 2 * i], H, W, g.tx, dir);
      SR_HIP_CHECK_LAUNCH();
    } else {
      if (!dst) dst = cur;
      if ((rc = c64_conv_t<T>(cur, nullptr, other, blob + boff[1 + 2 * i], N, H, W, 64, 1, st, nullptr, dir))) return rc;
      if ((rc = c64_conv_t<T>(other, cur, dst, blob + boff[2 + 2 * i], N, H, W, 64, 0, st, nullptr, dir))) return rc;
    }
    cur = dst;
  }
  return 0;
}
}  // namespace

extern "C" int sr_c64_trunk_fwd(const void* x0, const sr_c3_warp_t* warp, void* ping, void* pong, void* out, const void* blob,
                                const long* blob_off, int nb, int N, int H, int W, int ci0, int dtype, int n_dir,
                                long blob_dir_stride, sr_stream_t stream) {
  if ((!x0) == (!warp) || !out || (nb > 0 && (!ping || !pong || ping == pong || ping == out || pong == out)) || !blob || !blob_off ||
      nb < 0 || N <= 0 || H <= 0 || W <= 0 || N > 65535)
    return -2;
  if (ci0 != 64 && ci0 != 80) return -2;
  if (dtype != SR_DTYPE_BF16 && dtype != SR_DTYPE_F32) return -2;
  if (warp && (!warp->frame || ci0 != 80 || (warp->flow && !warp->state) || warp->dstate || warp->dflow || warp->x0_save ||
               (warp->state && warp->state == out)))
    return -2;
  if (n_dir < 0 || n_dir >= N || (n_dir > 0 && blob_dir_stride <= 0)) return -2;
  const C3Dir dir{blob_dir_stride, n_dir};
  return dtype == SR_DTYPE_BF16 ? c64_trunk_fwd_t<__bf16>(x0, warp, ping, pong, out, blob, blob_off, nb, N, H, W, ci0, (hipStream_t)stream, dir)
                                : c64_trunk_fwd_t<float>(x0, warp, ping, pong, out, blob, blob_off, nb, N, H, W, ci0, (hipStream_t)stream, dir);
}

// ------------------------------------------------------------------------------------------
// 64-feature propagation trunk, the opt-in training route (csrc/conv64.h forward kernels, csrc/conv64_bwd.h)
// ------------------------------------------------------------------------------------------
namespace {
// conv0 -> a_0; per block c64_conv<ReLU> -> t_i, c64_conv<none, +a_i> -> a_{i+1} (both dtypes: the two-launch form, whose result
// c64_resblock_kernel reproduces bit for bit)
template <typename T>
int c64_trunk_train_fwd_t(const void* x0, const sr_c3_warp_t* warp, void* acts_, void* mids_, const void* blob_, const long* boff,
                          int nb, int N, int H, int W, int ci0, hipStream_t st, C3Dir dir) {
  const size_t act = (size_t)N * H * W * 64;
  T* acts = (T*)acts_; T* mids = (T*)mids_; const T* blob = (const T*)blob_;
  int rc;
  if ((rc = c64_conv_t<T>(x0, nullptr, acts, blob + boff[0], N, H, W, ci0, 2, st, warp, dir))) return rc;
  for (int i = 0; i < nb; ++i) {
    if ((rc = c64_conv_t<T>(acts + i * act, nullptr, mids + i * act, blob + boff[1 + 2 * i], N, H, W, 64, 1, st, nullptr, dir))) return rc;
    if ((rc = c64_conv_t<T>(mids + i * act, acts + i * act, acts + (i + 1) * act, blob + boff[2 + 2 * i], N, H, W, 64, 0, st, nullptr, dir)))
      return rc;
  }
  return 0;
}

template <typename T>
int c64_wgrad_t(const void* x, const void* dA, const void* A, float* partial, int wgs, int N, int H, int W, int CI, int act,
                hipStream_t st, int layers, long x_ls, long d_ls, long a_ls, long p_ls, int n_dir) {
  const C3Grid g = c3_grid(N, H, W);
#define L(CI_, ACT_) hipLaunchKernelGGL((c64_wgrad_kernel<T, CI_, ACT_>), dim3(wgs, layers), dim3(C64Wg::NTHREADS), 0, st, (const T*)x, (const T*)dA, (const T*)A, partial, N, H, W, g.tx, g.tpi, x_ls, d_ls, a_ls, p_ls, n_dir)
  if (CI == 80 && act == 2) L(80, 2);
  else if (CI == 64 && act == 2) L(64, 2);
  else if (CI == 64 && act == 1) L(64, 1);
  else if (CI == 64 && act == 0) L(64, 0);
  else return -1;
#undef L
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int c64_warp_dflow_t(const void* g, const void* state, const float* flow, long flow_bs, float* dflow, long dflow_bs, int N, int H,
                     int W, hipStream_t st) {
  const int blocks = (int)(((long)H * W + C64Dflow::PX - 1) / C64Dflow::PX);
  hipLaunchKernelGGL((c64_warp_dflow_kernel<T>), dim3(blocks, N), dim3(C64Dflow::NTHREADS), 0, st, (const T*)g, (const T*)state, flow,
                     flow_bs, dflow, dflow_bs, H, W);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

// boff[k], k = 0..2nb: conv k's backward blob (conv 0: the state / plain-input half); boff[1 + 2nb]: conv 0's frame half, < 0 = not wanted
template <typename T>
int c64_trunk_bwd_t(const void* x0, const sr_c3_warp_t* warp, const void* acts_, const void* mids_, void* ga_, void* gt_,
                    const void* blob_, const long* boff, float* parts, void* dx0, const sr_c3_unpack_t* up, int nb, int wgs, int N,
                    int H, int W, int ci0, hipStream_t st, C3Dir dir) {
  const size_t act = (size_t)N * H * W * 64;
  const T* acts = (const T*)acts_; const T* mids = (const T*)mids_; const T* blob = (const T*)blob_;
  T* ga = (T*)ga_; T* gt = (T*)gt_;
  int rc;
  for (int i = nb - 1; i >= 0; --i) {                // a_{i+1} = a_i + conv2(t_i), t_i = relu(conv1(a_i))
    if ((rc = c64_conv_t<T>(ga + (i + 1) * act, nullptr, gt + i * act, blob + boff[2 + 2 * i], N, H, W, 64, 0, st, nullptr, dir))) return rc;
    if ((rc = c64_conv_t<T>(gt + i * act, ga + (i + 1) * act, ga + i * act, blob + boff[1 + 2 * i], N, H, W, 64, 0, st, nullptr, dir,
                            mids + i * act, 1)))
      return rc;
  }
  if (dx0) {                                         // dx0 = conv0^T(ga_0 * lrelu'(a_0)): [N,H,W,64] state / plain part, then the frame part
    if ((rc = c64_conv_t<T>(ga, nullptr, dx0, blob + boff[0], N, H, W, 64, 0, st, nullptr, dir, acts, 2))) return rc;
    if (ci0 == 80 && boff[1 + 2 * nb] >= 0 &&
        (rc = c64_conv_t<T>(ga, nullptr, (T*)dx0 + act, blob + boff[1 + 2 * nb], N, H, W, 64, 0, st, nullptr, dir, acts, 2)))
      return rc;
  }
  if (warp && warp->dstate) {                        // flow_warp backward, gather form (no float atomics)
    const int tx = (W + C3WarpBwd::TS - 1) / C3WarpBwd::TS, ty = (H + C3WarpBwd::TS - 1) / C3WarpBwd::TS;
    hipLaunchKernelGGL((c64_warp_bwd_kernel<T>), dim3(tx * ty, N, 4), dim3(256), 0, st, (const T*)dx0, warp->flow, warp->flow_bs,
                       warp->flow_bound, (T*)warp->dstate, H, W, tx);
    SR_HIP_CHECK_LAUNCH();
  }
  if (warp && warp->dflow) {                         // the flow's gradient (flow_training): per output pixel, reads dx0's state half
    if ((rc = c64_warp_dflow_t<T>(dx0, warp->state, warp->flow, warp->flow_bs, warp->dflow, warp->dflow_bs, N, H, W, st))) return rc;
  }
  if (!parts) return 0;
  const long s0 = C64Wg::slab(ci0), s1 = C64Wg::slab(64);
  float* const parts1 = parts + (size_t)wgs * s0;     // conv k >= 1: parts1 + (k - 1) wgs s1
  if (nb > 0) {                                      // every conv2, then every conv1, one launch each
    if ((rc = c64_wgrad_t<T>(mids, ga + act, ga + act, parts1 + (size_t)wgs * s1, wgs, N, H, W, 64, 0, st, nb, (long)act, (long)act,
                             (long)act, 2 * wgs * s1, dir.n_dir)))
      return rc;
    if ((rc = c64_wgrad_t<T>(acts, gt, mids, parts1, wgs, N, H, W, 64, 1, st, nb, (long)act, (long)act, (long)act, 2 * wgs * s1,
                             dir.n_dir)))
      return rc;
  }
  if ((rc = c64_wgrad_t<T>(warp ? warp->x0_save : x0, ga, acts, parts, wgs, N, H, W, ci0, 2, st, 1, 0, 0, 0, 0, dir.n_dir))) return rc;
  if (up) {                                          // slabs -> gradient of the flat parameter (of each trunk: its half of the slabs)
    UnpackSegs us;
    const int ndir = dir.n_dir > 0 ? 2 : 1, wd = wgs / ndir;
    const long total = (long)up->n0 + (nb > 0 ? 2L * nb * up->n1 : 0);
    us.nseg = 0;
    int blk = 0;
    for (int d = 0; d < ndir; ++d) {
      us.s[us.nseg++] = UnpackSeg{parts + (size_t)d * wd * s0, up->sidx0, up->dst0, d * total, 0, s0, wd, up->n0, 1, blk, wgs};
      blk += unpack_blocks(up->n0, wd);
      if (nb > 0) {
        us.s[us.nseg++] = UnpackSeg{parts1 + (size_t)d * wd * s1, up->sidx1, up->dst1, d * total + (long)up->n0, (long)up->n1, s1, wd,
                                    up->n1, 2 * nb, blk, wgs};
        blk += 2 * nb * unpack_blocks(up->n1, wd);
      }
    }
    hipLaunchKernelGGL(unpack_all_kernel, dim3(blk), dim3(64 * UNPACK_Q), 0, st, up->gflat, us);
    SR_HIP_CHECK_LAUNCH();
  }
  return 0;
}
}  // namespace

extern "C" int sr_c64_trunk_train_fwd(const void* x0, const sr_c3_warp_t* warp, void* acts, void* mids, const void* blob,
                                      const long* blob_off, int nb, int N, int H, int W, int ci0, int dtype, int n_dir,
                                      long blob_dir_stride, sr_stream_t stream) {
  if ((!x0) == (!warp) || !acts || (nb > 0 && !mids) || !blob || !blob_off || nb < 0 || N <= 0 || H <= 0 || W <= 0 || N > 65535) return -2;
  if (ci0 != 64 && ci0 != 80) return -2;
  if (dtype != SR_DTYPE_BF16 && dtype != SR_DTYPE_F32) return -2;
  if (warp && (!warp->frame || ci0 != 80 || (warp->flow && !warp->state) || warp->dstate || warp->dflow)) return -2;
  if (n_dir < 0 || n_dir >= N || (n_dir > 0 && blob_dir_stride <= 0)) return -2;
  const C3Dir dir{blob_dir_stride, n_dir};
  return dtype == SR_DTYPE_BF16 ? c64_trunk_train_fwd_t<__bf16>(x0, warp, acts, mids, blob, blob_off, nb, N, H, W, ci0, (hipStream_t)stream, dir)
                                : c64_trunk_train_fwd_t<float>(x0, warp, acts, mids, blob, blob_off, nb, N, H, W, ci0, (hipStream_t)stream, dir);
}
extern "C" int sr_c64_trunk_bwd(const void* x0, const sr_c3_warp_t* warp, const void* acts, const void* mids, void* ga, void* gt,
                                const void* bwd_blob, const long* bwd_blob_off, float* parts, void* dx0, const sr_c3_unpack_t* unpack,
                                int nb, int wgs, int N, int H, int W, int ci0, int dtype, int n_dir, long bwd_dir_stride,
                                sr_stream_t stream) {
  if ((!x0) == (!warp) || !acts || !ga || (nb > 0 && (!mids || !gt)) || !bwd_blob || !bwd_blob_off || nb < 0 || N <= 0 || H <= 0 ||
      W <= 0 || N > 65535)
    return -2;
  if (ci0 != 64 && ci0 != 80) return -2;
  if (dtype != SR_DTYPE_BF16 && dtype != SR_DTYPE_F32) return -2;
  if (warp && (!warp->frame || ci0 != 80 || (warp->flow && !warp->state))) return -2;
  if (warp && warp->dflow && (!dx0 || !warp->state || !warp->flow || (long)H * W > (1L << 30))) return -2;
  if (warp && warp->dstate && (!dx0 || !warp->state || (warp->flow && !warp->flow_bound))) return -2;
  if (parts && (wgs <= 0 || (warp && !warp->x0_save))) return -2;       // the weight gradient reads the input the forward kept
  if (unpack && (!parts || !unpack->sidx0 || !unpack->dst0 || !unpack->gflat || unpack->n0 <= 0 ||
                 (nb > 0 && (!unpack->sidx1 || !unpack->dst1 || unpack->n1 <= 0))))
    return -2;
  if (n_dir < 0 || n_dir >= N || (n_dir > 0 && (bwd_dir_stride <= 0 || (parts && (wgs & 1))))) return -2;
  const C3Dir dir{bwd_dir_stride, n_dir};
  return dtype == SR_DTYPE_BF16
             ? c64_trunk_bwd_t<__bf16>(x0, warp, acts, mids, ga, gt, bwd_blob, bwd_blob_off, parts, dx0, unpack, nb, wgs, N, H, W, ci0, (hipStream_t)stream, dir)
             : c64_trunk_bwd_t<float>(x0, warp, acts, mids, ga, gt, bwd_blob, bwd_blob_off, parts, dx0, unpack, nb, wgs, N, H, W, ci0, (hipStream_t)stream, dir);
}

// the flow gradient of the gathered first conv alone (c64_warp_dflow_kernel): what sr_c64_trunk_bwd launches for warp->dflow
extern "C" int sr_c64_warp_dflow(const void* g, const void* state, const float* flow, long flow_bs, float* dflow, long dflow_bs,
                                 int N, int H, int W, int dtype, sr_stream_t stream) {
  if (!g || !state || !flow || !dflow || N <= 0 || H <= 0 || W <= 0 || N > 65535 || (long)H * W > (1L << 30)) return -2;
  if (dtype != SR_DTYPE_BF16 && dtype != SR_DTYPE_F32) return -2;
  return dtype == SR_DTYPE_BF16 ? c64_warp_dflow_t<__bf16>(g, state, flow, flow_bs, dflow, dflow_bs, N, H, W, (hipStream_t)stream)
                                : c64_warp_dflow_t<float>(g, state, flow, flow_bs, dflow, dflow_bs, N, H, W, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------
// reconstruction of BasicVSR_origin, inference (csrc/vsr_recon.h)
// ------------------------------------------------------------------------------------------
namespace {
template <typename T>
int c64_recon_fwd_t(const void* fb, const void* ff, int cw, const float* frame, long frame_bs, const void* blob_, const long* boff,
                    void* fused, void* up1, void* up2, void* hr, float* out, long out_bs, int N, int H, int W, int stages,
                    hipStream_t st) {
  const T* blob = (const T*)blob_;
  const dim3 blk(C64Cfg::NTHREADS);
  if (stages & 1) {
    const C3Grid g = c3_grid(N, H, W);
    hipLaunchKernelGGL((vr_fusion_kernel<T>), g.grid, blk, 0, st, (const T*)fb, (const T*)ff, cw, (T*)fused, blob + boff[0], H, W, g.tx);
    SR_HIP_CHECK_LAUNCH();
  }
  if (stages & 2) {
    const C3Grid g = c3_grid(N, H, W);
    hipLaunchKernelGGL((vr_upconv_kernel<T>), g.grid, blk, 0, st, (const T*)fused, (T*)up1, blob + boff[1], H, W, g.tx);
    SR_HIP_CHECK_LAUNCH();
  }
  if (stages & 4) {
    const C3Grid g = c3_grid(N, 2 * H, 2 * W);
    hipLaunchKernelGGL((vr_upconv_kernel<T>), g.grid, blk, 0, st, (const T*)up1, (T*)up2, blob + boff[2], 2 * H, 2 * W, g.tx);
    SR_HIP_CHECK_LAUNCH();
  }
  if (stages & 8) {
    const int rc = c64_conv_t<T>(up2, nullptr, hr, blob + boff[3], N, 4 * H, 4 * W, 64, 2, st, nullptr, C3Dir{0, 0});
    if (rc) return rc;
  }
  if (stages & 16) {
    const C3Grid g = c3_grid(N, 4 * H, 4 * W);
    hipLaunchKernelGGL((vr_last_kernel<T>), g.grid, blk, 0, st, (const T*)hr, blob + boff[4], frame, frame_bs, out, out_bs, 4 * H,
                       4 * W, g.tx);
    SR_HIP_CHECK_LAUNCH();
  }
  return 0;
}
}  // namespace

extern "C" int sr_c64_recon_fwd(const void* feat_b, const void* feat_f, int cw, const float* frame, long frame_bs, const void* blob,
                                const long* blob_off, void* fused, void* up1, void* up2, void* hr, float* out, long out_bs, int N,
                                int H, int W, int dtype, int stages, sr_stream_t stream) {
  if (!blob || !blob_off || N <= 0 || H <= 0 || W <= 0 || N > 65535 || H > 8192 || W > 8192) return -2;
  if (dtype != SR_DTYPE_BF16 && dtype != SR_DTYPE_F32) return -2;
  if (stages <= 0 || stages > 31) return -2;
  if ((stages & 1) && (!feat_b || !feat_f || !fused || (cw != 24 && cw != 64))) return -2;
  if ((stages & 2) && (!fused || !up1 || fused == up1)) return -2;
  if ((stages & 4) && (!up1 || !up2 || up1 == up2)) return -2;
  if ((stages & 8) && (!up2 || !hr || up2 == hr)) return -2;
  if ((stages & 16) && (!hr || !frame || !out || frame_bs < 3L * H * W || out_bs < 48L * H * W)) return -2;
  for (int k = 0; k < 5; ++k)
    if (blob_off[k] < 0 || (blob_off[k] & 7)) return -2;         // 16-byte aligned fragments in either dtype
  return dtype == SR_DTYPE_BF16
             ? c64_recon_fwd_t<__bf16>(feat_b, feat_f, cw, frame, frame_bs, blob, blob_off, fused, up1, up2, hr, out, out_bs, N, H, W, stages, (hipStream_t)stream)
             : c64_recon_fwd_t<float>(feat_b, feat_f, cw, frame, frame_bs, blob, blob_off, fused, up1, up2, hr, out, out_bs, N, H, W, stages, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------
// reconstruction of BasicVSR_origin, backward of the opt-in training route (csrc/vsr_recon_bwd.h)
// ------------------------------------------------------------------------------------------
namespace {
int vr_sec_wgs(int wgs, int N, int H, int W) {
  const long tiles = (long)N * ((H + 15) / 16) * ((W + 15) / 16);
  return (int)std::min<long>(wgs, tiles);
}
// the four sub-convs of an upconv in one launch: blockIdx.y = q, dz through the stride-2 view of the 2H x 2W images
template <typename T>
int vr_up_wgrad_t(const void* x, const void* dA, const void* A, float* partial, int wgs, int grid, int N, int H, int W, hipStream_t st) {
  const C3Grid g = c3_grid(N, H, W);
  hipLaunchKernelGGL((c64_wgrad_kernel<T, 64, 2, 1>), dim3(grid, 4), dim3(C64Wg::NTHREADS), 0, st, (const T*)x, (const T*)dA, (const T*)A,
                     partial, N, H, W, g.tx, g.tpi, 0L, 0L, 0L, (long)wgs * VRBwd::WSLAB, 0);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int c64_recon_bwd_t(const void* fb, const void* ff, const void* fused, const void* up1, const void* up2, const void* hr, const float* g,
                    long g_bs, const void* blob_, const long* boff, void* d_hr, void* d_up2, void* d_up1, void* d_fused, void* dfb,
                    void* dff, float* parts, int wgs, int N, int H, int W, int stages, hipStream_t st) {
  const T* blob = (const T*)blob_;
  const dim3 blk(C64Cfg::NTHREADS);
  const C3Dir nodir{0, 0};
  auto sec = [&](int k) { return parts + (size_t)k * wgs * VRBwd::WSLAB; };
  // a section's launch has min(wgs, tiles) workgroups (a workgroup without a tile would only store zeros); the reduction sums as many
  const int e0 = vr_sec_wgs(wgs, N, H, W), e1 = vr_sec_wgs(wgs, N, 2 * H, 2 * W), e2 = vr_sec_wgs(wgs, N, 4 * H, 4 * W);
  int rc;
  if (stages & 16) {                                   // conv_last
    const C3Grid g4 = c3_grid(N, 4 * H, 4 * W);
    hipLaunchKernelGGL((vr_last_bwd_kernel<T>), g4.grid, blk, 0, st, g, g_bs, (const T*)hr, blob + boff[5], (T*)d_hr, 4 * H, 4 * W, g4.tx);
    SR_HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL((vr_last_wgrad_kernel<T>), dim3(e2), blk, 0, st, g, g_bs, (const T*)hr, sec(VRBwd::NSEC), N, 4 * H, 4 * W, g4.tx,
                       g4.tpi);
    SR_HIP_CHECK_LAUNCH();
  }
  if (stages & 8) {                                    // conv_hr: d_hr is masked already
    if ((rc = c64_conv_t<T>(d_hr, nullptr, d_up2, blob + boff[4], N, 4 * H, 4 * W, 64, 0, st, nullptr, nodir))) return rc;
    if ((rc = c64_wgrad_t<T>(up2, d_hr, d_hr, sec(10), e2, N, 4 * H, 4 * W, 64, 0, st, 1, 0, 0, 0, 0, 0))) return rc;
  }
  if (stages & 4) {                                    // upconv2: 2H x 2W -> 4H x 4W
    const C3Grid g2 = c3_grid(N, 2 * H, 2 * W);
    hipLaunchKernelGGL((vr_upconv_bwd_kernel<T>), g2.grid, blk, 0, st, (const T*)d_up2, (const T*)up2, (T*)d_up1, blob + boff[3], 2 * H,
                       2 * W, g2.tx);
    SR_HIP_CHECK_LAUNCH();
    if ((rc = vr_up_wgrad_t<T>(up1, d_up2, up2, sec(6), wgs, e1, N, 2 * H, 2 * W, st))) return rc;
  }
  if (stages & 2) {                                    // upconv1: H x W -> 2H x 2W
    const C3Grid g1 = c3_grid(N, H, W);
    hipLaunchKernelGGL((vr_upconv_bwd_kernel<T>), g1.grid, blk, 0, st, (const T*)d_up1, (const T*)up1, (T*)d_fused, blob + boff[2], H, W,
                       g1.tx);
    SR_HIP_CHECK_LAUNCH();
    if ((rc = vr_up_wgrad_t<T>(fused, d_up1, up1, sec(2), wgs, e0, N, H, W, st))) return rc;
  }
  if (stages & 1) {                                    // fusion: the 1x1 conv as the centre tap of a 3x3 one, once per trunk
    if ((rc = c64_conv_t<T>(d_fused, nullptr, dfb, blob + boff[0], N, H, W, 64, 0, st, nullptr, nodir, fused, 2))) return rc;
    if ((rc = c64_conv_t<T>(d_fused, nullptr, dff, blob + boff[1], N, H, W, 64, 0, st, nullptr, nodir, fused, 2))) return rc;
    if ((rc = c64_wgrad_t<T>(fb, d_fused, fused, sec(0), e0, N, H, W, 64, 2, st, 1, 0, 0, 0, 0, 0))) return rc;
    if ((rc = c64_wgrad_t<T>(ff, d_fused, fused, sec(1), e0, N, H, W, 64, 2, st, 1, 0, 0, 0, 0, 0))) return rc;
  }
  return 0;
}
}  // namespace

extern "C" int sr_c64_recon_bwd_slab(void) { return (int)VRBwd::per_wg(); }

extern "C" int sr_c64_recon_bwd(const void* feat_b, const void* feat_f, const void* fused, const void* up1, const void* up2,
                                const void* hr, const float* g, long g_bs, const void* bwd_blob, const long* blob_off, void* d_hr,
                                void* d_up2, void* d_up1, void* d_fused, void* dfeat_b, void* dfeat_f, float* parts, int wgs, int N,
                                int H, int W, int dtype, int stages, sr_stream_t stream) {
  if (!bwd_blob || !blob_off || !parts || N <= 0 || H <= 0 || W <= 0 || N > 65535 || H > 8192 || W > 8192) return -2;
  if (wgs < 1 || wgs > 1024) return -2;
  if (dtype != SR_DTYPE_BF16 && dtype != SR_DTYPE_F32) return -2;
  if (stages <= 0 || stages > 31) return -2;
  if ((stages & 16) && (!g || !hr || !d_hr || g_bs < 48L * H * W)) return -2;
  if ((stages & 8) && (!d_hr || !up2 || !d_up2 || d_hr == d_up2)) return -2;
  if ((stages & 4) && (!d_up2 || !up2 || !up1 || !d_up1)) return -2;
  if ((stages & 2) && (!d_up1 || !up1 || !fused || !d_fused)) return -2;
  if ((stages & 1) && (!d_fused || !fused || !feat_b || !feat_f || !dfeat_b || !dfeat_f || dfeat_b == dfeat_f || dfeat_b == d_fused ||
                       dfeat_f == d_fused))
    return -2;
  if (16L * N * ((4L * H + 15) / 16) * ((4L * W + 15) / 16) > 2147483647L) return -2;      // the tile walks count with an int
  for (int k = 0; k < 6; ++k)
    if (blob_off[k] < 0 || (blob_off[k] & 7)) return -2;
  return dtype == SR_DTYPE_BF16
             ? c64_recon_bwd_t<__bf16>(feat_b, feat_f, fused, up1, up2, hr, g, g_bs, bwd_blob, blob_off, d_hr, d_up2, d_up1, d_fused, dfeat_b, dfeat_f, parts, wgs, N, H, W, stages, (hipStream_t)stream)
             : c64_recon_bwd_t<float>(feat_b, feat_f, fused, up1, up2, hr, g, g_bs, bwd_blob, blob_off, d_hr, d_up2, d_up1, d_fused, dfeat_b, dfeat_f, parts, wgs, N, H, W, stages, (hipStream_t)stream);
}

extern "C" int sr_c64_recon_reduce(const float* parts, int wgs, const int* table, int n, float* grads, int accumulate, int N, int H,
                                   int W, sr_stream_t stream) {
  if (!parts || !table || !grads || n <= 0 || wgs < 1 || wgs > 1024 || N <= 0 || H <= 0 || W <= 0 || N > 65535 || H > 8192 || W > 8192)
    return -2;
  hipLaunchKernelGGL(vr_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, parts, table, grads, n, wgs,
                     vr_sec_wgs(wgs, N, H, W), vr_sec_wgs(wgs, N, 2 * H, 2 * W), vr_sec_wgs(wgs, N, 4 * H, 4 * W), accumulate ? 1 : 0);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------
// reconstruction of MotionVectorVSR, forward and backward (csrc/mv_recon.h)
// ------------------------------------------------------------------------------------------
namespace {
template <typename T, int CW>
int mv_recon_fwd_t(const void* const* fb, const void* const* ff, const float* x, long x_bs, long x_fs, const void* blob, float* out,
                   long out_bs, long out_fs, void* u_save, int NF, int B, int H, int W, hipStream_t st) {
  typedef MVCfg<T, CW> C;
  const int tiles_x = (W + C::TW - 1) / C::TW, tiles = tiles_x * ((H + C::TH - 1) / C::TH);
  for (int f0 = 0; f0 < NF; f0 += 16) {
    const int nf = std::min(16, NF - f0);
    MVPtrs p{};
    for (int i = 0; i < nf; ++i) {
      p.fb[i] = fb[f0 + i];
      p.ff[i] = ff[f0 + i];
    }
    hipLaunchKernelGGL((mv_recon_fwd_kernel<T, CW>), dim3(tiles, B, nf), dim3(C::NT), 0, st, p, (const T*)blob, x, x_bs, x_fs, out,
                       out_bs, out_fs, (T*)u_save, f0, B, H, W, tiles_x);
    SR_HIP_CHECK_LAUNCH();
  }
  return 0;
}
template <typename T>
int mv_recon_bwd_t(const void* const* fb, const void* const* ff, const void* u_save, const float* g, long g_bs, long g_fs,
                   const void* blob, void* const* dfb, void* const* dff, float* parts, int wgs, float* grads, int F, int NF, int B,
                   int H, int W, hipStream_t st) {
  typedef MVCfg<T, 24> C;
  const int tiles_x = (W + C::TW - 1) / C::TW, tiles = tiles_x * ((H + C::TH - 1) / C::TH);
  int nslabs = 0;
  for (int f0 = 0; f0 < NF; f0 += 16) {
    const int nf = std::min(16, NF - f0);
    MVPtrs p{};
    MVGPtrs gp{};
    for (int i = 0; i < nf; ++i) {
      p.fb[i] = fb[f0 + i];
      p.ff[i] = ff[f0 + i];
      gp.dfb[i] = dfb[f0 + i];
      gp.dff[i] = dff[f0 + i];
    }
    const long items = (long)nf * B * tiles;
    const int grid = (int)std::min<long>(items, wgs);
    hipLaunchKernelGGL((mv_recon_bwd_kernel<T>), dim3(grid), dim3(C::NT), 0, st, p, gp, (const T*)blob, (const T*)u_save, g, g_bs,
                       g_fs, parts + (size_t)nslabs * C::SLAB, f0, nf, B, H, W, tiles_x, tiles);
    SR_HIP_CHECK_LAUNCH();
    nslabs += grid;
  }
  const int total = 4 * F * F + 2 * F + 150 * F + 3;
  hipLaunchKernelGGL(mv_recon_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, st, (const float*)parts, nslabs, grads, F);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
}  // namespace

extern "C" int sr_mv_recon_slab(void) { return MVCfg<float, 24>::SLAB; }

extern "C" int sr_mv_recon_fwd(const void* const* feat_b, const void* const* feat_f, int cw, const float* x, long x_bs, long x_fs,
                               const void* blob, float* out, long out_bs, long out_fs, void* u_save, int NF, int B, int H, int W,
                               int dtype, sr_stream_t stream) {
  if (!feat_b || !feat_f || !x || !blob || !out || NF <= 0 || B <= 0 || H <= 0 || W <= 0 || B > 65535 || H > 8192 || W > 8192) return -2;
  if (dtype != SR_DTYPE_BF16 && dtype != SR_DTYPE_F32) return -2;
  if (cw != 24 && cw != 64) return -2;
  if (x_fs < 3L * H * W || x_bs < x_fs || out_fs < 48L * H * W || out_bs < out_fs) return -2;
  for (int i = 0; i < NF; ++i)
    if (!feat_b[i] || !feat_f[i]) return -2;
  hipStream_t st = (hipStream_t)stream;
#define CALL(T, CW_) return mv_recon_fwd_t<T, CW_>(feat_b, feat_f, x, x_bs, x_fs, blob, out, out_bs, out_fs, u_save, NF, B, H, W, st);
  if (dtype == SR_DTYPE_BF16) { if (cw == 24) { CALL(__bf16, 24) } else { CALL(__bf16, 64) } }
  if (cw == 24) { CALL(float, 24) } else { CALL(float, 64) }
#undef CALL
}

extern "C" int sr_mv_recon_bwd(const void* const* feat_b, const void* const* feat_f, const void* u_save, const float* g, long g_bs,
                               long g_fs, const void* blob, void* const* dfeat_b, void* const* dfeat_f, float* parts, int wgs,
                               float* grads, int F, int NF, int B, int H, int W, int dtype, sr_stream_t stream) {
  if (!feat_b || !feat_f || !u_save || !g || !blob || !dfeat_b || !dfeat_f || !parts || !grads) return -2;
  if (NF <= 0 || B <= 0 || H <= 0 || W <= 0 || B > 65535 || H > 8192 || W > 8192 || F < 1 || F > 24 || wgs < 1 || wgs > 1024) return -2;
  if (dtype != SR_DTYPE_BF16 && dtype != SR_DTYPE_F32) return -2;
  if (g_fs < 48L * H * W || g_bs < g_fs) return -2;
  {                                                    // the kernel walks frames x clips x tiles of a 16-frame chunk with an int
    const long tiles = (long)((W + 15) / 16) * ((H + 7) / 8);
    if (16L * B * tiles > 2147483647L) return -2;
  }
  for (int i = 0; i < NF; ++i)
    if (!feat_b[i] || !feat_f[i] || !dfeat_b[i] || !dfeat_f[i]) return -2;
  hipStream_t st = (hipStream_t)stream;
  return dtype == SR_DTYPE_BF16
             ? mv_recon_bwd_t<__bf16>(feat_b, feat_f, u_save, g, g_bs, g_fs, blob, dfeat_b, dfeat_f, parts, wgs, grads, F, NF, B, H, W, st)
             : mv_recon_bwd_t<float>(feat_b, feat_f, u_save, g, g_bs, g_fs, blob, dfeat_b, dfeat_f, parts, wgs, grads, F, NF, B, H, W, st);
}

// the backward at cw = 64 (24 < F <= 64): mv_recon_bwd64_kernel + mv_recon_reduce64_kernel, blob = packing.mv_recon_bwd_tables
namespace {
template <typename T>
int mv_recon_bwd64_t(const void* const* fb, const void* const* ff, const void* u_save, const float* g, long g_bs, long g_fs,
                     const void* blob, void* const* dfb, void* const* dff, float* parts, int wgs, float* grads, int F, int NF, int B,
                     int H, int W, hipStream_t st) {
  typedef MVCfg<T, 64> C;
  const int tiles_x = (W + C::TW - 1) / C::TW, tiles = tiles_x * ((H + C::TH - 1) / C::TH);
  int nslabs = 0;
  for (int f0 = 0; f0 < NF; f0 += 16) {
    const int nf = std::min(16, NF - f0);
    MVPtrs p{};
    MVGPtrs gp{};
    for (int i = 0; i < nf; ++i) {
      p.fb[i] = fb[f0 + i];
      p.ff[i] = ff[f0 + i];
      gp.dfb[i] = dfb[f0 + i];
      gp.dff[i] = dff[f0 + i];
    }
    const long items = (long)nf * B * tiles;
    const int grid = (int)std::min<long>(items, wgs);
    hipLaunchKernelGGL((mv_recon_bwd64_kernel<T>), dim3(grid), dim3(C::NT), 0, st, p, gp, (const T*)blob, (const T*)u_save, g, g_bs,
                       g_fs, parts + (size_t)nslabs * C::SLAB64, f0, nf, B, H, W, tiles_x, tiles);
    SR_HIP_CHECK_LAUNCH();
    nslabs += grid;
  }
  const int total = 4 * F * F + 2 * F + 150 * F + 3;
  hipLaunchKernelGGL(mv_recon_reduce64_kernel, dim3((total + 255) / 256), dim3(256), 0, st, (const float*)parts, nslabs, grads, F);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
}  // namespace

extern "C" int sr_mv_recon_slab64(void) { return MVCfg<float, 64>::SLAB64; }

extern "C" int sr_mv_recon_bwd64(const void* const* feat_b, const void* const* feat_f, const void* u_save, const float* g, long g_bs,
                                 long g_fs, const void* blob, void* const* dfeat_b, void* const* dfeat_f, float* parts, int wgs,
                                 float* grads, int F, int NF, int B, int H, int W, int dtype, sr_stream_t stream) {
  if (!feat_b || !feat_f || !u_save || !g || !blob || !dfeat_b || !dfeat_f || !parts || !grads) return -2;
  if (NF <= 0 || B <= 0 || H <= 0 || W <= 0 || B > 65535 || H > 8192 || W > 8192 || F < 25 || F > 64 || wgs < 1 || wgs > 1024) return -2;
  if (dtype != SR_DTYPE_BF16 && dtype != SR_DTYPE_F32) return -2;
  if (g_fs < 48L * H * W || g_bs < g_fs) return -2;
  {                                                    // the kernel walks frames x clips x tiles of a 16-frame chunk with an int
    const long tiles = (long)((W + 15) / 16) * ((H + 3) / 4);      // the fp32 tile, the smaller of the two
    if (16L * B * tiles > 2147483647L) return -2;
  }
  for (int i = 0; i < NF; ++i)
    if (!feat_b[i] || !feat_f[i] || !dfeat_b[i] || !dfeat_f[i]) return -2;
  hipStream_t st = (hipStream_t)stream;
  return dtype == SR_DTYPE_BF16
             ? mv_recon_bwd64_t<__bf16>(feat_b, feat_f, u_save, g, g_bs, g_fs, blob, dfeat_b, dfeat_f, parts, wgs, grads, F, NF, B, H, W, st)
             : mv_recon_bwd64_t<float>(feat_b, feat_f, u_save, g, g_bs, g_fs, blob, dfeat_b, dfeat_f, parts, wgs, grads, F, NF, B, H, W, st);
}

// ------------------------------------------------------------------------------------------
// flow_warp
// ------------------------------------------------------------------------------------------
extern "C" int sr_flow_warp_fwd(const float* x, const float* flow, float* out, int N, int C, int H, int W,
                                sr_stream_t stream) {
  if (!x || !flow || !out || N <= 0 || C <= 0 || H <= 0 || W <= 0 || N > 65535) return -2;
  const int blocks = std::min((H * W + 15) / 16, 8192);          // one wave = 16 pixels x 4 channel phases
  hipLaunchKernelGGL(flow_warp_fwd_kernel, dim3(blocks, N), dim3(64), 0, (hipStream_t)stream, x, flow, out, C, H, W);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
extern "C" int sr_flow_warp_bwd(const float* x, const float* flow, const float* gout, float* dx, float* dflow, int N,
                                int C, int H, int W, sr_stream_t stream) {
  if (!x || !flow || !gout || N <= 0 || C <= 0 || H <= 0 || W <= 0 || N > 65535) return -2;
  const int blocks = std::min((H * W + 15) / 16, 8192);
  hipLaunchKernelGGL(flow_warp_bwd_kernel, dim3(blocks, N), dim3(64), 0, (hipStream_t)stream, x, flow, gout, dx, dflow,
                     C, H, W);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------
// NAS supernet block
// ------------------------------------------------------------------------------------------
#define SR_NAS_DISPATCH(CALL)                                                                   \
  if (F == 24 && dtype == SR_DTYPE_BF16) { CALL(__bf16, 24) } else if (F == 24 && dtype == SR_DTYPE_F32) { CALL(float, 24) } \
  else if (F == 32 && dtype == SR_DTYPE_BF16) { CALL(__bf16, 32) } else if (F == 32 && dtype == SR_DTYPE_F32) { CALL(float, 32) } \
  else return -1;
// the generic depthwise kernels: the fp32 parity route (bf16 runs the lane = channel kernels of csrc/nas_dw_lc.h)
#define SR_NAS_DISPATCH_F32(CALL)                                                               \
  if (F == 24 && dtype == SR_DTYPE_F32) { CALL(float, 24) } else if (F == 32 && dtype == SR_DTYPE_F32) { CALL(float, 32) } \
  else return -1;

extern "C" int sr_nas_dw_fwd(const void* yin, void* V, const float* dwp, int N, int H, int W, int F, int dtype,
                             sr_stream_t stream) {
  if (!yin || !V || !dwp || N <= 0 || H <= 0 || W <= 0 || N > 65535) return -2;
  hipStream_t st = (hipStream_t)stream;
  const long vs = (long)N * H * W * F;
  if (dtype == SR_DTYPE_BF16) {                        // lane = channel, packed bf16 dot products (csrc/nas_dw_lc.h)
    typedef NasCfg<24> C;
    const int tx = (W + C::TW - 1) / C::TW;
    dim3 g(tx * ((H + C::TH - 1) / C::TH), N);
    if (F == 24) hipLaunchKernelGGL((nas_dw_fwd_lc_kernel<24>), g, dim3(512), 0, st, (const __bf16*)yin, (__bf16*)V, dwp, H, W, tx, vs);
    else if (F == 32) hipLaunchKernelGGL((nas_dw_fwd_lc_kernel<32>), g, dim3(512), 0, st, (const __bf16*)yin, (__bf16*)V, dwp, H, W, tx, vs);
    else return -1;
    SR_HIP_CHECK_LAUNCH();
    return 0;
  }
#define CALL(T, F_) { typedef NasCfg<F_> C; const int tx = (W + C::TW - 1) / C::TW; dim3 g(tx * ((H + C::TH - 1) / C::TH), N); \
    hipLaunchKernelGGL((nas_dw_fwd_kernel<T, F_>), g, dim3(512), 0, st, (const T*)yin, (T*)V, dwp, H, W, tx, vs); }
  SR_NAS_DISPATCH_F32(CALL)
#undef CALL
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
extern "C" int sr_nas_pw_fwd(const void* yin, const void* V, void* y, const void* frags, const float* tabs,
                             const float* scal, int N, int H, int W, int F, int dtype, sr_stream_t stream) {
  if (!yin || !V || !y || !frags || !tabs || !scal || N <= 0 || H <= 0 || W <= 0 || N > 65535) return -2;
  hipStream_t st = (hipStream_t)stream;
  const long vs = (long)N * H * W * F;
#define CALL(T, F_) { typedef NasCfg<F_> C; const int tx = (W + C::TW - 1) / C::TW; dim3 g(tx * ((H + C::TH - 1) / C::TH), N); \
    hipLaunchKernelGGL((nas_pw_fwd_kernel<T, F_>), g, dim3(576), 0, st, (const T*)yin, (const T*)V, (T*)y, (const T*)frags, tabs, scal, H, W, tx, vs); }
  SR_NAS_DISPATCH(CALL)
#undef CALL
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
extern "C" int sr_nas_pw_bwd(const void* yin, const void* V, const void* gy, void* GZ, const void* frags,
                             const float* tabs, const float* scal, float* partial, int wgs, int N, int H, int W, int F,
                             int dtype, sr_stream_t stream) {
  if (!yin || !V || !gy || !GZ || !frags || !tabs || !scal || !partial || wgs <= 0 || N <= 0 || H <= 0 || W <= 0) return -2;
  hipStream_t st = (hipStream_t)stream;
  const long vs = (long)N * H * W * F;
#define CALL(T, F_) { typedef NasCfg<F_> C; const int tx = (W + C::TW - 1) / C::TW, tpi = tx * ((H + C::TH - 1) / C::TH); \
    hipLaunchKernelGGL((nas_pw_bwd_kernel<T, F_>), dim3(wgs), dim3(NasPwb<T>::THREADS), 0, st, (const T*)yin, (const T*)V, (const T*)gy, (T*)GZ, (const T*)frags, tabs, scal, partial, N, H, W, tx, tpi, vs); }
  SR_NAS_DISPATCH(CALL)
#undef CALL
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
extern "C" int sr_nas_dw_bwd(const void* yin, const void* GZ, const void* gy, void* gyin, const float* dwp,
                             float* partial, int wgs, int N, int H, int W, int F, int dtype, sr_stream_t stream) {
  if (!yin || !GZ || !gy || !gyin || !dwp || !partial || wgs <= 0 || N <= 0 || H <= 0 || W <= 0) return -2;
  hipStream_t st = (hipStream_t)stream;
  const long vs = (long)N * H * W * F;
  if (dtype == SR_DTYPE_BF16) {                        // lane = channel (csrc/nas_dw_lc.h); the dW part of the slab is sr_nas_dw_wgrad's
    typedef NasCfg<24> C;
    const int tx = (W + C::TW - 1) / C::TW, tpi = tx * ((H + C::TH - 1) / C::TH);
    if (F == 24) hipLaunchKernelGGL((nas_dw_bwd_lc_kernel<24>), dim3(wgs), dim3(NAS_DW_BWD_THREADS), 0, st, (const __bf16*)yin, (const __bf16*)GZ, (const __bf16*)gy, (__bf16*)gyin, dwp, partial, N, H, W, tx, tpi, vs);
    else if (F == 32) hipLaunchKernelGGL((nas_dw_bwd_lc_kernel<32>), dim3(wgs), dim3(NAS_DW_BWD_THREADS), 0, st, (const __bf16*)yin, (const __bf16*)GZ, (const __bf16*)gy, (__bf16*)gyin, dwp, partial, N, H, W, tx, tpi, vs);
    else return -1;
    SR_HIP_CHECK_LAUNCH();
    return 0;
  }
#define CALL(T, F_) { typedef NasCfg<F_> C; const int tx = (W + C::TW - 1) / C::TW, tpi = tx * ((H + C::TH - 1) / C::TH); \
    hipLaunchKernelGGL((nas_dw_bwd_kernel<T, F_>), dim3(wgs), dim3(512), 0, st, (const T*)yin, (const T*)GZ, (const T*)gy, (T*)gyin, dwp, partial, N, H, W, tx, tpi, vs); }
  SR_NAS_DISPATCH_F32(CALL)
#undef CALL
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

extern "C" int sr_nas_dw_wgrad(const void* yin, const void* GZ, const float* dwp, float* partial, int wgs, int N, int H,
                               int W, int F, int dtype, sr_stream_t stream) {
  if (!yin || !GZ || !dwp || !partial || wgs <= 0 || N <= 0 || H <= 0 || W <= 0) return -2;
  hipStream_t st = (hipStream_t)stream;
  const long vs = (long)N * H * W * F;
  if (dtype == SR_DTYPE_BF16) {                        // the three stencils from one workgroup per tile
    typedef NasCfg<24> C;
    const int tx = (W + C::TW - 1) / C::TW, tpi = tx * ((H + C::TH - 1) / C::TH);
    if (F == 24) hipLaunchKernelGGL((nas_dw_wgrad3_kernel<24>), dim3(wgs), dim3(768), 0, st, (const __bf16*)yin, (const __bf16*)GZ, dwp, partial, N, H, W, tx, tpi, vs);
    else if (F == 32) hipLaunchKernelGGL((nas_dw_wgrad3_kernel<32>), dim3(wgs), dim3(768), 0, st, (const __bf16*)yin, (const __bf16*)GZ, dwp, partial, N, H, W, tx, tpi, vs);
    else return -1;
    SR_HIP_CHECK_LAUNCH();
    return 0;
  }
#define CALL(T, F_) { typedef NasCfg<F_> C; const int tx = (W + C::TW - 1) / C::TW, tpi = tx * ((H + C::TH - 1) / C::TH); \
    hipLaunchKernelGGL((nas_dw_wgrad_kernel<T, F_>), dim3(wgs, 3), dim3(768), 0, st, (const T*)yin, (const T*)GZ, dwp, partial, N, H, W, tx, tpi, vs); }
  SR_NAS_DISPATCH_F32(CALL)
#undef CALL
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------
// whole network
// ------------------------------------------------------------------------------------------
namespace {
template <typename T> int net_pack(const sr_wdsr_net_t* n, hipStream_t st) {
  const int cb = (n->n_chan + 3) / 4, bb = (n->n_bias + 255) / 256;
  hipLaunchKernelGGL(wn_src_kernel, dim3(cb + bb), dim3(256), 0, st, n->flat, n->src, (const int4*)n->chan_tab,
                     n->n_chan, n->bias_tab, n->bias_const, n->n_bias, cb);
  PackSegs ps;
  ps.nseg = 4;
  int blk = 0;
  auto add = [&](int k, const int* idx, void* out, long off, long stride, int cnt, int reps, int as_float) {
    ps.s[k] = PackSeg{idx, out, off, stride, cnt, reps, as_float, blk};
    blk += reps * ((cnt + 255) / 256);
  };
  add(0, n->idx_head, n->blob_head, n->src_head_off, 0, n->n_idx_head, 1, 0);
  add(1, n->idx_body, n->blob_body, n->src_body_off, n->src_body_stride, n->n_idx_body, n->NB, 0);
  add(2, n->idx_cinit, n->cinit_body, n->src_body_off, n->src_body_stride, n->n_idx_cinit, n->NB, 1);
  add(3, n->idx_tail, n->blob_tail, n->src_tail_off, 0, n->n_idx_tail, 1, 0);
  hipLaunchKernelGGL((pack_all_kernel<T>), dim3(blk), dim3(256), 0, st, n->src, ps);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
}  // namespace

// t / dt of every block are kept for the weight-gradient kernels when every block runs through the
// two-block kernels (bf16, F = 24, even block count) and the caller provided both buffers
static bool net_saves_side_images(const sr_wdsr_net_t* n, bool backward) {
  return (n->F == 24 || n->F == 32) && n->dtype == SR_DTYPE_BF16 && n->tsave && (!backward || n->dtsave);
}
// Two blocks per launch pay while a launch is bound by its fixed costs (about one workgroup per CU); with more
// workgroups the single-block kernels win (two resident per CU, no halo-2 recompute): measured crossover at
// batch 64 of 48x48 patches = 512 workgroups (tools/bench_rows.py).
static long net_tiles(const sr_wdsr_net_t* n) {
  const Tiles t = block_tiles(n->H, n->W);
  return (long)n->N * t.x * t.y;
}
// The forward and the backward both decide here, from the same fields of the net struct.  32 units: n->one_block32 keeps the
// one-block kernels (the parity tests compare the two forms).
static bool net_uses_pairs(const sr_wdsr_net_t* n) {
  return n->dtype == SR_DTYPE_BF16 && net_tiles(n) <= 384 && (n->F == 24 || (n->F == 32 && !n->one_block32));
}
// The training step (sr_wdsr_net_train_step) runs the tail once, forward + loss + backward in one launch (sr_tail_train):
// the forward then stops after the last block (SR_NET_SKIP_TAIL) and the backward starts with that launch.
static bool net_step_fuses_tail(const sr_wdsr_net_t* n) {
  return n->dtype == SR_DTYPE_BF16 && n->R == 4 && (n->F == 24 || n->F == 32) && n->hr && n->N <= 65535;
}
static size_t side_image_bytes(const sr_wdsr_net_t* n) {     // one block's [N][tiles][288][LP] image
  typedef WdsrDims<24>::Cfg C;
  const Tiles t = block_tiles<C>(n->H, n->W);
  const int lp = n->F == 24 ? C::LP : WdsrDims<32>::Cfg::LP;
  return (size_t)n->N * ((size_t)t.x * t.y) * C::TH * C::TW * lp * 2;
}
// Block i's slices of the buffers a net struct points to, every offset formed in size_t: NetView{n, keeps_side}
struct NetView {
  const sr_wdsr_net_t* n;
  bool keeps_side;                                           // this call writes or reads the t / dt images
  size_t esz = n->dtype == SR_DTYPE_BF16 ? 2 : 4;
  size_t act_bytes = (size_t)n->N * n->H * n->W * n->F * esz, blob_bytes = (size_t)n->n_idx_body * esz;
  size_t side_bytes = side_image_bytes(n);
  char* act(int i) const { return (char*)n->acts + (size_t)i * act_bytes; }         // input of block i; NB: input of the tail
  char* grad(int i) const { return (char*)n->grads + (size_t)i * act_bytes; }       // gradient of act(i)
  char* blob(int i) const { return (char*)n->blob_body + (size_t)i * blob_bytes; }
  const float* cinit(int i) const { return n->cinit_body + (size_t)i * n->n_idx_cinit; }
  char* tsave(int i) const { return keeps_side ? (char*)n->tsave + (size_t)i * side_bytes : nullptr; }
  char* dtsave(int i) const { return keeps_side ? (char*)n->dtsave + (size_t)i * side_bytes : nullptr; }
};

extern "C" int sr_wdsr_net_forward(const sr_wdsr_net_t* n, int flags, sr_stream_t stream) {
  if (!n || !n->flat || !n->src) return -2;
  if (!(flags & SR_NET_PACK_ONLY) && (!n->x || !n->acts || !n->out)) return -2;
  hipStream_t st = (hipStream_t)stream;
  const int save_acts = flags & SR_NET_SAVE_ACTS;
  int rc = 0;
  if (!(flags & SR_NET_WEIGHTS_PACKED)) rc = n->dtype == SR_DTYPE_BF16 ? net_pack<__bf16>(n, st) : net_pack<float>(n, st);
  if (rc || (flags & SR_NET_PACK_ONLY)) return rc;
  const NetView v{n, save_acts && net_saves_side_images(n, false)};
  char* acts = v.act(0);
  if ((rc = sr_head_fwd(n->x, acts, n->blob_head, n->mean, n->N, n->H, n->W, n->F, n->dtype, stream))) return rc;
  char* cur = acts;
  // inference over many tiles per CU: the persistent two-block launches (csrc/wdsr_fwd_rs.h) beat the single-block ones
  // again (0.29 vs 0.27 of the roof at batch 512); with saved images (training) the large grids stay on single blocks
  // 32 units: two blocks per launch at launch-bound grids only (the sixteen-wave kernel)
  const bool pairs = net_uses_pairs(n) || (n->F == 24 && n->dtype == SR_DTYPE_BF16 &&
                                           ((!save_acts && net_tiles(n) >= 768) || fwd_stream_applies(n->N, n->H, n->W)));
  for (int i = 0, nb; i < n->NB; i += nb) {
    nb = pairs && i + 1 < n->NB ? 2 : 1;           // blocks of this launch
    char* nxt = save_acts ? v.act(i + nb) : (cur == acts ? v.act(1) : acts);   // inference keeps nothing: two slots in turn
    if (nb == 2)
      rc = sr_wdsr_block2_fwd(cur, save_acts ? v.act(i + 1) : nullptr, nxt, v.blob(i), v.blob(i + 1), v.cinit(i), v.cinit(i + 1),
                              v.tsave(i), v.tsave(i + 1), n->N, n->H, n->W, n->F, n->dtype, stream);
    else if (pairs)                                // odd block count at a launch-bound grid: same kernel family, one block
      rc = sr_wdsr_fwd_rs(cur, nullptr, nxt, v.blob(i), nullptr, v.cinit(i), nullptr, v.tsave(i), nullptr, 1, n->N, n->H, n->W, n->F,
                          n->dtype, stream);
    else if (v.keeps_side)                         // single-block kernel that also keeps t (bf16)
      rc = dispatch_f(n->F, [&](auto d) {
        return launch_block_fwd<__bf16, decltype(d)::F>(cur, nxt, v.blob(i), v.cinit(i), n->N, n->H, n->W, st, v.tsave(i));
      });
    else
      rc = sr_wdsr_block_fwd(cur, nxt, v.blob(i), v.cinit(i), n->N, n->H, n->W, n->F, n->dtype, stream);
    if (rc) return rc;
    cur = nxt;
  }
  if (flags & SR_NET_SKIP_TAIL) return 0;          // the caller's next launch is sr_tail_train on act(NB)
  return sr_tail_fwd(cur, n->x, n->out, n->blob_tail, n->mean, n->N, n->H, n->W, n->F, n->R, n->dtype, stream);
}

// Backward in up to two parts so that the gradient of the LATE parameters (blocks [nb_split, NB), tail, skip) is final --
// bucket-ready for a DistributedDataParallel all-reduce -- before the early half (head, blocks [0, nb_split)) runs.
//   part 0: everything (one call);  part 1: late half;  part 2: early half (after part 1).
namespace {
struct FusedAdam { float* m; float* v; AdamArgs a; const float* loss_part; int n_loss; float loss_scale; float* loss_out; };
}
// fa != nullptr (part 0 only): the weight-norm backward also applies the Adam step (wn_bwd_adam_kernel)
// tail_train (part 0 only): the forward stopped after the last block; the tail runs here, forward + loss + backward
static int net_backward_part_impl(const sr_wdsr_net_t* n, int part, sr_stream_t stream, const FusedAdam* fa, bool tail_train = false) {
  if (!n || !n->flat || !n->gflat || !n->dsrc || !n->x || !n->acts || !n->grads || part < 0 || part > 2) return -2;
  if (tail_train && (part != 0 || !n->hr)) return -2;
  if (part != 2 && (n->hr ? ((!n->out && !tail_train) || !n->loss_part || (n->loss_kind != 1 && n->loss_kind != 2)) : !n->dout)) return -2;
  hipStream_t st = (hipStream_t)stream;
  const long act_e = (long)n->N * n->H * n->W * n->F;
  const bool pairs = net_uses_pairs(n);
  const bool saved = net_saves_side_images(n, true);
  const NetView v{n, saved};
  int split = part == 0 ? 0 : n->nb_split;
  if (part != 0 && (split <= 0 || split >= n->NB || (pairs && ((n->NB - split) & 1)))) return -2;   // (pair launches must not straddle the split)
  const int b0 = part == 1 ? split : 0, b1 = part == 2 ? split : n->NB;      // blocks [b0, b1) handled by this call
  int rc;
  if (part != 2) {
    if (tail_train)
      rc = sr_tail_train(n->hr, n->loss_kind, n->loss_gscale, n->loss_part, v.act(n->NB), n->x, n->mean, n->blob_tail, v.grad(n->NB),
                         n->part_tail, n->wgs_tail, n->N, n->H, n->W, n->F, n->R, n->dtype, stream);
    else if (n->hr)                                 // loss folded into the tail backward: no HR gradient tensor
      rc = sr_tail_bwd_loss(n->out, n->hr, n->loss_kind, n->loss_gscale, n->loss_part, v.act(n->NB), n->x, n->mean, n->blob_tail,
                            v.grad(n->NB), n->part_tail, n->wgs_tail, n->N, n->H, n->W, n->F, n->R, n->dtype, stream);
    else if (n->dtype == SR_DTYPE_BF16)             // data + weight gradients of the tail in one launch
      rc = sr_tail_bwd(n->dout, v.act(n->NB), n->x, n->mean, n->blob_tail, v.grad(n->NB), n->part_tail, n->wgs_tail, n->N, n->H, n->W,
                       n->F, n->R, n->dtype, stream);
    else if (!(rc = sr_tail_bwd_data(n->dout, v.grad(n->NB), n->blob_tail, n->N, n->H, n->W, n->F, n->R, n->dtype, stream)))
      rc = sr_tail_wgrad(n->dout, v.act(n->NB), n->x, n->mean, n->part_tail, n->wgs_tail, n->N, n->H, n->W, n->F, n->R, n->dtype,
                         stream);
    if (rc) return rc;
  }
  for (int i = b1 - 1, nb; i >= b0; i -= nb) {
    nb = pairs && i >= b0 + 1 ? 2 : 1;             // blocks of this launch
    if (nb == 2)
      rc = sr_wdsr_block2_bwd_data(v.act(i - 1), v.act(i), v.grad(i + 1), v.grad(i), v.grad(i - 1), v.blob(i - 1), v.blob(i),
                                   v.cinit(i - 1), v.cinit(i), v.dtsave(i - 1), v.dtsave(i), n->N, n->H, n->W, n->F, n->dtype, stream);
    else if (saved)
      rc = dispatch_f(n->F, [&](auto d) {
        return launch_block_bwd_data<__bf16, decltype(d)::F>(v.act(i), v.grad(i + 1), v.grad(i), v.blob(i), v.cinit(i), n->N, n->H,
                                                                 n->W, st, v.dtsave(i));
      });
    else
      rc = sr_wdsr_block_bwd_data(v.act(i), v.grad(i + 1), v.grad(i), v.blob(i), v.cinit(i), n->N, n->H, n->W, n->F, n->dtype, stream);
    if (rc) return rc;
  }
  // weight gradients of blocks [b0, b1): every per-layer pointer advanced by b0 layers
  const int nl = b1 - b0;
  const int wgs_part = nl > 0 ? (n->wgs_body * n->NB) / nl : 0;
  if (nl > 0) {
    float* pa0 = n->part_a;                         // a part owns the whole partial-slab buffer while it runs, so a
    float* pb0 = n->part_b;                         // half-depth part spreads each layer over twice the workgroups
    if (saved)
      rc = sr_wdsr_block_wgrad_saved(v.act(b0), v.grad(b0 + 1), v.tsave(b0), v.dtsave(b0), v.blob(b0), v.cinit(b0), pa0, pb0, nl,
                                     wgs_part, n->N, n->H, n->W, n->F, n->dtype, act_e, act_e, (long)(v.side_bytes / v.esz),
                                     (long)n->n_idx_body, (long)n->n_idx_cinit, stream);
    else
      rc = sr_wdsr_block_wgrad(v.act(b0), v.grad(b0 + 1), v.blob(b0), v.cinit(b0), pa0, pb0, nl, wgs_part, n->N, n->H, n->W, n->F,
                               n->dtype, act_e, act_e, (long)n->n_idx_body, (long)n->n_idx_cinit, stream);
    if (rc) return rc;
  }
  if (part != 1)
    if ((rc = sr_head_wgrad(v.grad(0), n->x, n->mean, n->part_head, n->wgs_head, n->N, n->H, n->W, n->F, n->dtype, stream)))
      return rc;
  // slabs -> d(effective weights) -> d(flat parameters), for the layers of this part
  {
    UnpackSegs us;
    us.nseg = 0;
    int blk = 0;
    auto add = [&](const float* part_, const int* sidx, const int* dst, long off, long stride, long slab, int wgs, int cnt,
                   int reps) {
      us.s[us.nseg++] = UnpackSeg{part_, sidx, dst, off, stride, slab, wgs, cnt, reps, blk};
      blk += reps * unpack_blocks(cnt, wgs);
    };
    if (nl > 0) {
      add(n->part_a, n->ga_sidx, n->ga_dst, n->src_body_off + b0 * n->src_body_stride, n->src_body_stride, n->slab_a, wgs_part,
          n->n_ga, nl);
      add(n->part_b, n->gb_sidx, n->gb_dst, n->src_body_off + b0 * n->src_body_stride, n->src_body_stride, n->slab_b, wgs_part,
          n->n_gb, nl);
    }
    if (part != 2) add(n->part_tail, n->gt_sidx, n->gt_dst, n->src_tail_off, 0, n->slab_tail, n->wgs_tail, n->n_gt, 1);
    if (part != 1) add(n->part_head, n->gh_sidx, n->gh_dst, n->src_head_off, 0, n->slab_head, n->wgs_head, n->n_gh, 1);
    hipLaunchKernelGGL(unpack_all_kernel, dim3(blk), dim3(64 * UNPACK_Q), 0, st, n->dsrc, us);
  }
  // weight-norm backward over the table rows of this part (rows are in state_dict order: head, body.0 .., tail, skip)
  const int c0 = part == 1 ? n->chan_split : 0, c1 = part == 2 ? n->chan_split : n->n_chan;
  const int d0 = part == 1 ? n->bias_split : 0, d1 = part == 2 ? n->bias_split : n->n_bias;
  const int cb = (c1 - c0 + 3) / 4, bb = (d1 - d0 + 255) / 256;
  if (fa)
    hipLaunchKernelGGL(wn_bwd_adam_kernel, dim3(cb + bb), dim3(256), 0, st, const_cast<float*>(n->flat), n->dsrc, n->gflat, fa->m, fa->v,
                       (const int4*)n->chan_tab + c0, c1 - c0, n->bias_tab + 3 * d0, d1 - d0, cb, fa->a, fa->loss_part, fa->n_loss,
                       fa->loss_scale, fa->loss_out);
  else
    hipLaunchKernelGGL(wn_bwd_kernel, dim3(cb + bb), dim3(256), 0, st, n->flat, n->dsrc, n->gflat, (const int4*)n->chan_tab + c0,
                       c1 - c0, n->bias_tab + 3 * d0, d1 - d0, cb);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
extern "C" int sr_wdsr_net_backward_part(const sr_wdsr_net_t* n, int part, sr_stream_t stream) {
  return net_backward_part_impl(n, part, stream, nullptr);
}

extern "C" int sr_wdsr_net_backward(const sr_wdsr_net_t* n, sr_stream_t stream) { return sr_wdsr_net_backward_part(n, 0, stream); }

// table-driven parameter plumbing for callers other than the BASIC_MODEL net struct (the supernet body)
extern "C" int sr_param_pack(const float* flat, float* src, const int* chan_tab, int n_chan, const int* bias_tab,
                             const float* bias_const, int n_bias, const sr_pack_seg_t* segs, int nseg, int dtype,
                             sr_stream_t stream) {
  if (!flat || !src || !chan_tab || n_chan <= 0 || n_bias < 0 || (n_bias > 0 && (!bias_tab || !bias_const)) || !segs || nseg < 1 ||
      nseg > 4 || (dtype != SR_DTYPE_F32 && dtype != SR_DTYPE_BF16))
    return -2;
  hipStream_t st = (hipStream_t)stream;
  PackSegs ps;                                       // every segment is validated before the first launch: a refused call writes nothing
  ps.nseg = nseg;
  int blk = 0;
  for (int k = 0; k < nseg; ++k) {
    const sr_pack_seg_t& g = segs[k];
    if (!g.idx || !g.out || g.n <= 0 || g.reps <= 0) return -2;
    ps.s[k] = PackSeg{g.idx, g.out, g.src_off, g.src_stride, g.n, g.reps, g.as_float, blk};
    blk += g.reps * ((g.n + 255) / 256);
  }
  const int cb = (n_chan + 3) / 4, bb = (n_bias + 255) / 256;
  hipLaunchKernelGGL(wn_src_kernel, dim3(cb + bb), dim3(256), 0, st, flat, src, (const int4*)chan_tab, n_chan, bias_tab, bias_const,
                     n_bias, cb);
  if (dtype == SR_DTYPE_BF16) hipLaunchKernelGGL((pack_all_kernel<__bf16>), dim3(blk), dim3(256), 0, st, src, ps);
  else hipLaunchKernelGGL((pack_all_kernel<float>), dim3(blk), dim3(256), 0, st, src, ps);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

extern "C" int sr_param_grads(const float* flat, float* dsrc, float* gflat, const int* chan_tab, int n_chan, const int* bias_tab,
                              int n_bias, const sr_unpack_seg_t* segs, int nseg, sr_stream_t stream) {
  if (!flat || !dsrc || !gflat || !chan_tab || n_chan <= 0 || n_bias < 0 || (n_bias > 0 && !bias_tab) || !segs || nseg < 1 || nseg > 4)
    return -2;
  hipStream_t st = (hipStream_t)stream;
  UnpackSegs us;
  us.nseg = nseg;
  int blk = 0;
  for (int k = 0; k < nseg; ++k) {
    const sr_unpack_seg_t& g = segs[k];
    if (!g.partial || !g.sidx || !g.dst || g.n <= 0 || g.reps <= 0 || g.wgs <= 0) return -2;
    us.s[k] = UnpackSeg{g.partial, g.sidx, g.dst, g.dst_off, g.dst_stride, g.slab, g.wgs, g.n, g.reps, blk};
    blk += g.reps * unpack_blocks(g.n, g.wgs);
  }
  hipLaunchKernelGGL(unpack_all_kernel, dim3(blk), dim3(64 * UNPACK_Q), 0, st, dsrc, us);
  const int cb = (n_chan + 3) / 4, bb = (n_bias + 255) / 256;
  hipLaunchKernelGGL(wn_bwd_kernel, dim3(cb + bb), dim3(256), 0, st, flat, dsrc, gflat, (const int4*)chan_tab, n_chan, bias_tab,
                     n_bias, cb);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

extern "C" int sr_nas_scalars(const float* mask_w, const float* split_w, const float* alpha, const float* alpha1,
                              const float* alpha2, int nb, int F, float* out, float* src, long src_stride, int off_mg, float* scal,
                              sr_stream_t stream) {
  if (!mask_w || !split_w || !alpha || !alpha1 || !alpha2 || !out || nb <= 0 || F < 8 || (src && (src_stride <= 0 || off_mg < 0)))
    return -2;
  if ((long)(nb + 1) * F > NAS_SCALARS_MAX) return -1;
  hipLaunchKernelGGL(nas_scalars_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, mask_w, split_w, alpha, alpha1, alpha2, nb,
                     F, out, src, src_stride, off_mg, scal);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

extern "C" int sr_nas_mask_grads(const float* dsrc, long ds, int off_r, int off_sxy, int off_sA, int off_sB, const float* ms,
                                 const float* p, const float* beta, int nb, int F, float* out, sr_stream_t stream) {
  if (!dsrc || !ms || !p || !beta || !out || nb <= 0 || nb > 1024 || F <= 0 || ds <= 0) return -2;
  hipLaunchKernelGGL(nas_mask_grads_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, dsrc, ds, off_r, off_sxy, off_sA, off_sB, ms,
                     p, beta, nb, F, out);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

// every block of the supernet body from one call each way
extern "C" int sr_nas_body_fwd(void* ys, void* V, const float* dwp, long dwp_bs, const void* frags, long frags_bs, const float* tabs,
                               long tabs_bs, const float* scal, long scal_bs, int nb, int N, int H, int W, int F, int dtype,
                               int split, sr_stream_t stream) {
  if (!ys || !V || !dwp || !frags || !tabs || !scal || nb <= 0 || N <= 0 || H <= 0 || W <= 0) return -2;
  const size_t act = (size_t)N * H * W * F * (dtype == SR_DTYPE_BF16 ? 2 : 4);
  // bf16: depthwise + pointwise of a block from one launch (csrc/nas_dw_lc.h nas_block_fwd_kernel); split != 0: the two kernels
  const bool fused = dtype == SR_DTYPE_BF16 && (F == 24 || F == 32) && N <= 65535 && !split;
  for (int i = 0; i < nb; ++i) {
    char* yi = (char*)ys + (size_t)i * act;
    char* Vi = (char*)V + (size_t)i * 3 * act;
    int rc;
    if (fused) {
      typedef NasCfg<24> C;
      const int tx = (W + C::TW - 1) / C::TW;
      const dim3 g(tx * ((H + C::TH - 1) / C::TH), N);
      const long vs = (long)N * H * W * F;
      const float* dw_i = (const float*)((const char*)dwp + (size_t)i * dwp_bs);
      const __bf16* fr_i = (const __bf16*)((const char*)frags + (size_t)i * frags_bs);
      const float* tb_i = (const float*)((const char*)tabs + (size_t)i * tabs_bs);
      const float* sc_i = (const float*)((const char*)scal + (size_t)i * scal_bs);
      hipStream_t st = (hipStream_t)stream;
      if (F == 24) hipLaunchKernelGGL((nas_block_fwd_kernel<24>), g, dim3(NAS_BLOCK_FWD_THREADS), 0, st, (const __bf16*)yi, (__bf16*)Vi, (__bf16*)(yi + act), dw_i, fr_i, tb_i, sc_i, H, W, tx, vs);
      else hipLaunchKernelGGL((nas_block_fwd_kernel<32>), g, dim3(NAS_BLOCK_FWD_THREADS), 0, st, (const __bf16*)yi, (__bf16*)Vi, (__bf16*)(yi + act), dw_i, fr_i, tb_i, sc_i, H, W, tx, vs);
      SR_HIP_CHECK_LAUNCH();
      continue;
    }
    if ((rc = sr_nas_dw_fwd(yi, Vi, (const float*)((const char*)dwp + (size_t)i * dwp_bs), N, H, W, F, dtype, stream))) return rc;
    if ((rc = sr_nas_pw_fwd(yi, Vi, yi + act, (const char*)frags + (size_t)i * frags_bs, (const float*)((const char*)tabs + (size_t)i * tabs_bs),
                            (const float*)((const char*)scal + (size_t)i * scal_bs), N, H, W, F, dtype, stream)))
      return rc;
  }
  return 0;
}
extern "C" int sr_nas_body_bwd(const void* ys, const void* V, const void* g_out, void* g_tmp0, void* g_tmp1, void* GZ, const float* dwp,
                               long dwp_bs, const void* frags, long frags_bs, const float* tabs, long tabs_bs, const float* scal,
                               long scal_bs, float* part_pw, long pw_bs, float* part_dw, long dw_bs, int wgs, int nb, int N, int H,
                               int W, int F, int dtype, int split, void** g_in, sr_stream_t stream) {
  if (!ys || !V || !g_out || !g_tmp0 || !g_tmp1 || !GZ || !dwp || !frags || !tabs || !scal || !part_pw || !part_dw || !g_in || wgs <= 0 ||
      nb <= 0 || N <= 0 || H <= 0 || W <= 0)
    return -2;
  const size_t act = (size_t)N * H * W * F * (dtype == SR_DTYPE_BF16 ? 2 : 4);
  const void* g = g_out;
  // bf16, one tile per workgroup: csrc/nas_bwd_fused.h; split != 0: the separate kernels
  const int tx_f = (W + NasCfg<24>::TW - 1) / NasCfg<24>::TW, tpi_f = tx_f * ((H + NasCfg<24>::TH - 1) / NasCfg<24>::TH);
  const long vs_f = (long)N * H * W * F;
  const bool fused = dtype == SR_DTYPE_BF16 && (F == 24 || F == 32) && (long)N * tpi_f <= wgs && !split;
  for (int i = nb - 1; i >= 0; --i) {
    void* gin = (i & 1) ? g_tmp1 : g_tmp0;
    const char* yi = (const char*)ys + (size_t)i * act;
    const char* Vi = (const char*)V + (size_t)i * 3 * act;
    const float* dw_i = (const float*)((const char*)dwp + (size_t)i * dwp_bs);
    float* pdw = (float*)((char*)part_dw + (size_t)i * dw_bs);
    int rc;
    if (fused) {                                       // pointwise backward + depthwise weight gradients from one launch
      const float* tb_i = (const float*)((const char*)tabs + (size_t)i * tabs_bs);
      const float* sc_i = (const float*)((const char*)scal + (size_t)i * scal_bs);
      const __bf16* fr_i = (const __bf16*)((const char*)frags + (size_t)i * frags_bs);
      float* ppw = (float*)((char*)part_pw + (size_t)i * pw_bs);
      hipStream_t st = (hipStream_t)stream;
      if (F == 24) hipLaunchKernelGGL((nas_block_bwd_a_kernel<24>), dim3(wgs), dim3(768), 0, st, (const __bf16*)yi, (const __bf16*)Vi, (const __bf16*)g, (__bf16*)GZ, fr_i, tb_i, sc_i, dw_i, ppw, pdw, N, H, W, tx_f, tpi_f, vs_f);
      else hipLaunchKernelGGL((nas_block_bwd_a_kernel<32>), dim3(wgs), dim3(768), 0, st, (const __bf16*)yi, (const __bf16*)Vi, (const __bf16*)g, (__bf16*)GZ, fr_i, tb_i, sc_i, dw_i, ppw, pdw, N, H, W, tx_f, tpi_f, vs_f);
      SR_HIP_CHECK_LAUNCH();
      if ((rc = sr_nas_dw_bwd(yi, GZ, g, gin, dw_i, pdw, wgs, N, H, W, F, dtype, stream))) return rc;
      g = gin;
      continue;
    }
    if ((rc = sr_nas_pw_bwd(yi, Vi, g, GZ, (const char*)frags + (size_t)i * frags_bs, (const float*)((const char*)tabs + (size_t)i * tabs_bs),
                            (const float*)((const char*)scal + (size_t)i * scal_bs), (float*)((char*)part_pw + (size_t)i * pw_bs), wgs, N,
                            H, W, F, dtype, stream)))
      return rc;
    if ((rc = sr_nas_dw_bwd(yi, GZ, g, gin, dw_i, pdw, wgs, N, H, W, F, dtype, stream))) return rc;
    if ((rc = sr_nas_dw_wgrad(yi, GZ, dw_i, pdw, wgs, N, H, W, F, dtype, stream))) return rc;
    g = gin;
  }
  *g_in = const_cast<void*>(g);
  return 0;
}

// ------------------------------------------------------------------------------------------
// standalone PixelShuffle
// ------------------------------------------------------------------------------------------
extern "C" int sr_pixel_shuffle(const float* in, float* out, int N, int C, int H, int W, int r, int inverse, sr_stream_t stream) {
  if (!in || !out || N <= 0 || C <= 0 || H <= 0 || W <= 0 || r < 1 || r > 8) return -2;
  const long total4 = inverse ? (long)N * C * r * r * H * ((W + 3) / 4) : (long)N * C * (H * r) * ((W * r + 3) / 4);
  const long blocks = (total4 + 255) / 256;
  if (blocks > 0x7fffffffL) return -2;
  if (inverse)
    hipLaunchKernelGGL((pixel_shuffle_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, out, C, H, W, r, total4);
  else
    hipLaunchKernelGGL((pixel_shuffle_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, out, C, H, W, r, total4);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------
// input pipeline
// ------------------------------------------------------------------------------------------
extern "C" int sr_patch_gather(const unsigned char* cache, const void* recs, float* lr_out, float* hr_out, int B, int P, int scale,
                               sr_stream_t stream) {
  static_assert(sizeof(PatchRec) == 40, "record layout is part of the ABI (sr_patch_rec_t)");
  if (!cache || !recs || (!lr_out && !hr_out) || B <= 0 || B > 65535 || P <= 0 || scale <= 0) return -2;
  hipStream_t st = (hipStream_t)stream;
  if (lr_out) {
    const int blocks = std::min((3 * P * P + 255) / 256, 64);
    hipLaunchKernelGGL(sr_patch_gather_kernel, dim3(blocks, B), dim3(256), 0, st, cache, (const PatchRec*)recs, lr_out, P, scale, 0);
  }
  if (hr_out) {
    const int S = P * scale, blocks = std::min((3 * S * S + 255) / 256, 256);
    hipLaunchKernelGGL(sr_patch_gather_kernel, dim3(blocks, B), dim3(256), 0, st, cache, (const PatchRec*)recs, hr_out, P, scale, 1);
  }
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

extern "C" int sr_clip_gather(const unsigned char* cache, const float* mv_cache, const void* frames, const int* ids, const void* recs,
                              float* lr_out, float* hr_out, int B, int T, int P, int scale, sr_stream_t stream) {
  static_assert(sizeof(ClipRec) == 24 && sizeof(ClipRec) == sizeof(sr_clip_rec_t) && offsetof(ClipRec, x) == offsetof(sr_clip_rec_t, x) &&
                offsetof(ClipRec, T) == offsetof(sr_clip_rec_t, T), "record layout is part of the ABI (sr_clip_rec_t)");
  static_assert(sizeof(ClipFrame) == 32 && sizeof(ClipFrame) == sizeof(sr_clip_frame_t) &&
                offsetof(ClipFrame, mv_off) == offsetof(sr_clip_frame_t, mv_off) && offsetof(ClipFrame, hr_w) == offsetof(sr_clip_frame_t, hr_w),
                "frame table layout is part of the ABI (sr_clip_frame_t)");
  if (!cache || !frames || !ids || !recs || (!lr_out && !hr_out) || (mv_cache && !lr_out) || B <= 0 || T <= 0 ||
      (long)B * T > 65535 || P <= 0 || scale <= 0 || (long)P * scale > 8192 || ((uintptr_t)lr_out & 15) || ((uintptr_t)hr_out & 15) ||
      ((uintptr_t)mv_cache & 7))
    return -2;
  const int S = P * scale, RL = (P + clips::RUN - 1) / clips::RUN, RH = (S + clips::RUN - 1) / clips::RUN;
  const int items = (lr_out ? P * RL : 0) + (hr_out ? S * RH : 0);
  hipLaunchKernelGGL(sr_clip_gather_kernel, dim3(std::min((items + 255) / 256, 256), B * T), dim3(256), 0, (hipStream_t)stream, cache,
                     mv_cache, (const ClipFrame*)frames, ids, (const ClipRec*)recs, lr_out, hr_out, T, P, scale);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

static int bicubic_args_ok(int scale, const double* w, const int* idx, int taps) {
  return scale >= 2 && scale <= bicubic::MAX_SCALE && w && idx && taps >= 1 && taps <= bicubic::MAXT;
}

extern "C" int sr_bicubic_resize_u8(const unsigned char* img, unsigned char* out_u8, float* out_f32, float* src_f32, int H, int W, int scale,
                                    const double* wr, const int* ir, int taps_r, const double* wc, const int* ic, int taps_c,
                                    sr_stream_t stream) {
  if (scale < 2 || scale > bicubic::MAX_SCALE) return -1;
  if (!img || (!out_u8 && !out_f32) || H <= 0 || W <= 0 || !bicubic_args_ok(scale, wr, ir, taps_r) ||
      !bicubic_args_ok(scale, wc, ic, taps_c))
    return -2;
  const int Ho = (H + scale - 1) / scale, Wo = (W + scale - 1) / scale;
  const long tiles_x = (Wo + bicubic::TW - 1) / bicubic::TW, tiles = tiles_x * ((Ho + bicubic::TH - 1) / bicubic::TH);
  if (tiles > 0x7fffffffL) return -1;
  hipLaunchKernelGGL(sr_bicubic_resize_kernel, dim3((unsigned)tiles), dim3(bicubic::THREADS), 0, (hipStream_t)stream, img, out_u8,
                     out_f32, src_f32, H, W, Ho, Wo, wr, ir, taps_r, wc, ic, taps_c, (int)tiles_x);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

extern "C" int sr_bicubic_patch_gather(const unsigned char* cache, const void* recs, float* lr_out, float* hr_out, int B, int P,
                                       int scale, int ig, const double* w, const int* idx, int taps, sr_stream_t stream) {
  static_assert(sizeof(bicubic::Rec) == 24 && sizeof(bicubic::Rec) == sizeof(sr_bicubic_rec_t) &&
                offsetof(bicubic::Rec, w) == offsetof(sr_bicubic_rec_t, hr_w) &&
                offsetof(bicubic::Rec, flags) == offsetof(sr_bicubic_rec_t, flags), "record layout is part of the ABI (sr_bicubic_rec_t)");
  if (scale < 2 || scale > bicubic::MAX_SCALE) return -1;
  if (!cache || !recs || (!lr_out && !hr_out) || B <= 0 || B > 65535 || P <= 0 || ig < 1 || (long)(P + 2L * ig) * scale > 32768 ||
      !bicubic_args_ok(scale, w, idx, taps))
    return -2;
  const int tiles_x = (P + bicubic::TW - 1) / bicubic::TW;
  const int lr_tiles = lr_out ? tiles_x * ((P + bicubic::TH - 1) / bicubic::TH) : 0;
  const int HS = P * scale, hr_blocks = hr_out ? std::min((3 * HS * HS + bicubic::THREADS - 1) / bicubic::THREADS, 256) : 0;
  hipLaunchKernelGGL(sr_bicubic_patch_kernel, dim3(lr_tiles + hr_blocks, B), dim3(bicubic::THREADS), 0, (hipStream_t)stream, cache,
                     (const bicubic::Rec*)recs, lr_out, hr_out, P, scale, ig, w, idx, taps, lr_tiles, tiles_x);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------
// evaluation metrics
// ------------------------------------------------------------------------------------------
extern "C" int sr_psnr(const float* sr, const float* hr, float* partial, float* out, int N, int C, int H, int W, int shave,
                       int luma, int wgs, sr_stream_t stream) {
  if (!sr || !hr || !partial || !out || N <= 0 || C <= 0 || H <= 0 || W <= 0 || shave < 0 || wgs <= 0 || N > 65535 ||
      (luma && C != 3 && luma != -1))
    return -2;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(wgs, N);
  if (luma == 1) hipLaunchKernelGGL((sr_sqdiff_kernel<1>), grid, dim3(256), 0, st, sr, hr, partial, C, H, W, shave);
  else if (luma == -1) hipLaunchKernelGGL((sr_sqdiff_kernel<-1>), grid, dim3(256), 0, st, sr, hr, partial, C, H, W, shave);
  else hipLaunchKernelGGL((sr_sqdiff_kernel<0>), grid, dim3(256), 0, st, sr, hr, partial, C, H, W, shave);
  const long hs = H - 2 * shave, ws = W - 2 * shave;
  const double count = (hs > 0 && ws > 0) ? (double)hs * ws * (luma == 1 ? 1 : C) : 0.0;
  hipLaunchKernelGGL(sr_psnr_finish_kernel, dim3(1), dim3(64), 0, st, partial, out, N, wgs, count);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

extern "C" int sr_ssim(const float* sr, const float* hr, double* partial, double* out, int N, int H, int W, int shave,
                       long n_partial, sr_stream_t stream) {
  if (!sr || !hr || !partial || !out || N <= 0 || N > 65535 || H <= 0 || W <= 0 || shave < 1) return -2;
  const long ho = (long)H - 2L * shave - 2 * ssim::R, wo = (long)W - 2L * shave - 2 * ssim::R;   // output pixels per image
  if (ho < 1 || wo < 1) return -2;                                                               // a shaved side < 11
  const long tiles_x = (wo + ssim::TW - 1) / ssim::TW, tiles = tiles_x * ((ho + ssim::TH - 1) / ssim::TH);
  if (tiles > 0x7fffffffL) return -1;
  if (n_partial < tiles * N) return -2;
  ssim::Weights wt;                     // scipy's gaussian_filter1d kernel: sigma 1.5, truncate 3.5 -> radius 5
  double wsum = 0.0;
  for (int k = 0; k < ssim::TAPS; ++k) wsum += wt.w[k] = std::exp(-0.5 / (1.5 * 1.5) * (double)((k - ssim::R) * (k - ssim::R)));
  for (int k = 0; k < ssim::TAPS; ++k) wt.w[k] /= wsum;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sr_ssim_tile_kernel, dim3((unsigned)tiles, N), dim3(ssim::THREADS), 0, st, sr, hr, partial, H, W, shave,
                     (int)tiles_x, wt);
  hipLaunchKernelGGL(sr_ssim_finish_kernel, dim3(1), dim3(256), 0, st, partial, out, N, (int)tiles, (double)ho * (double)wo);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

// ATen's area_pixel_compute_scale for a resize given by its output SIZE (no scale factor), in float
static evalk::Resize eval_resize(int h, int w, int H, int W, int align_corners) {
  evalk::Resize r;
  r.h = h; r.w = w; r.align = align_corners ? 1 : 0;
  if (align_corners) {
    r.sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f;
    r.sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
  } else {
    r.sy = (float)h / (float)H;
    r.sx = (float)w / (float)W;
  }
  return r;
}
static int eval_side_ok(int v) { return v > 0 && v <= 32768; }

extern "C" int sr_eval_clip(const float* sr, const float* lr, const float* hr, float* partial, float* out, int F, int H, int W, int h,
                            int w, int lr_channels, int shave, int align_corners, int wgs, sr_stream_t stream) {
  if (!sr || !lr || !hr || !partial || !out || F <= 0 || F > 65535 || !eval_side_ok(H) || !eval_side_ok(W) || !eval_side_ok(h) ||
      !eval_side_ok(w) || lr_channels < 3 || shave < 0 || shave > 32768 || wgs <= 0 || wgs > 65535 || ((uintptr_t)partial & 15))
    return -2;
  hipStream_t st = (hipStream_t)stream;
  const int vec = W % 4 == 0 && !((uintptr_t)sr & 15) && !((uintptr_t)hr & 15);
  hipLaunchKernelGGL(eval_clip_kernel, dim3(wgs, F), dim3(256), 0, st, sr, lr, hr, partial, H, W, lr_channels,
                     eval_resize(h, w, H, W, align_corners), shave, vec);
  const long hs = (long)H - 2L * shave, ws = (long)W - 2L * shave;
  hipLaunchKernelGGL(eval_clip_finish_kernel, dim3(1), dim3(256), 0, st, partial, out, F, wgs,
                     (hs > 0 && ws > 0) ? (double)hs * (double)ws : 0.0, 3.0 * (double)H * (double)W);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

extern "C" int sr_eval_u8(const float* src, unsigned char* out, int F, int H, int W, int h, int w, int src_channels, int from_lr,
                          int align_corners, sr_stream_t stream) {
  if (!src || !out || F <= 0 || F > 65535 || !eval_side_ok(H) || !eval_side_ok(W) || ((uintptr_t)out & 3)) return -2;
  if (from_lr ? (!eval_side_ok(h) || !eval_side_ok(w) || src_channels < 3) : src_channels != 3) return -2;
  hipStream_t st = (hipStream_t)stream;
  const int items = H * (((W + 2) >> 2) + 1);
  const dim3 grid(std::max(1, std::min((items + 255) / 256, 96)), F);   // <= 96 workgroups per frame, grid-stride beyond
  if (from_lr) {
    hipLaunchKernelGGL((eval_u8_kernel<1>), grid, dim3(256), 0, st, src, out, H, W, src_channels,
                       eval_resize(h, w, H, W, align_corners), 0);
  } else {
    const int vec = W % 4 == 0 && !((uintptr_t)src & 15);
    hipLaunchKernelGGL((eval_u8_kernel<0>), grid, dim3(256), 0, st, src, out, H, W, 3, evalk::Resize{0.f, 0.f, 1, 1, 0}, vec);
  }
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

extern "C" int sr_eval_variation(const float* lr, float* partial, float* out, int B, int N, int C, int h, int w, int wgs,
                                 sr_stream_t stream) {
  if (!lr || !partial || !out || B <= 0 || N <= 0 || (long)B * N > 65535 || C <= 0 || !eval_side_ok(h) || !eval_side_ok(w) ||
      (long)C * h * w > (1L << 30) || wgs <= 0 || wgs > 65535)
    return -2;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(eval_variation_kernel, dim3(wgs, B * N), dim3(256), 0, st, lr, partial, N, C, h, w);
  hipLaunchKernelGGL(eval_variation_finish_kernel, dim3(1), dim3(256), 0, st, partial, out, B * N, N, wgs);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------
// loss / optimizer epilogue
// ------------------------------------------------------------------------------------------
extern "C" int sr_adam_step(float* p, const float* g, float* m, float* v, long n, const sr_adam_t* a, const float* loss_part,
                            int n_loss, float loss_scale, float* loss_out, sr_stream_t stream) {
  if (!p || !g || !m || !v || !a || n <= 0 || (loss_out && (!loss_part || n_loss <= 0))) return -2;
  const AdamArgs aa{a->w_lerp, a->beta2, a->one_minus_beta2, a->bc2_sqrt, a->eps, a->neg_step_size};
  const long blocks = (n + 1023) / 1024;
  hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, aa, loss_part, n_loss,
                     loss_scale, loss_out);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
static_assert(SR_ADAM_MULTI_CAP == ADAM_MULTI_CAP && SR_ADAM_MULTI_CHUNK == ADAM_MULTI_CHUNK, "sr_hotpath.h and train_step.h disagree");
extern "C" int sr_adam_step_multi(const sr_adam_row_t* rows, int count, const sr_adam_t* a, sr_stream_t stream) {
  if (!rows || !a || count < 1 || count > ADAM_MULTI_CAP) return -2;
  AdamTable t;
  long blocks = 0;
  for (int i = 0; i < count; ++i) {
    const sr_adam_row_t& r = rows[i];
    if (!r.param || !r.grad || !r.exp_avg || !r.exp_avg_sq || r.n <= 0) return -2;
    t.row[i] = AdamRow{r.param, r.grad, r.exp_avg, r.exp_avg_sq, r.n, (int)blocks, 0};
    blocks += (r.n + ADAM_MULTI_CHUNK - 1) / ADAM_MULTI_CHUNK;
    if (blocks > 2147483647L) return -1;
  }
  for (int i = count; i < ADAM_MULTI_CAP; ++i) t.row[i] = AdamRow{nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
  t.a = AdamArgs{a->w_lerp, a->beta2, a->one_minus_beta2, a->bc2_sqrt, a->eps, a->neg_step_size};
  t.count = count;
  t.pad = 0;
  hipLaunchKernelGGL(adam_step_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, t);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
extern "C" int sr_loss_value(const float* loss_part, int n_loss, float loss_scale, float* loss_out, sr_stream_t stream) {
  if (!loss_part || !loss_out || n_loss <= 0) return -2;
  hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, loss_part, n_loss, loss_scale, loss_out);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
extern "C" int sr_scale_by(void* y, const void* x, long n, const float* scale, int dtype, sr_stream_t stream) {
  if (!y || !x || !scale || n <= 0 || ((uintptr_t)y & 15) || ((uintptr_t)x & 15)) return -2;
  const unsigned blocks = (unsigned)((n + 2047) / 2048);
  if (dtype == SR_DTYPE_BF16)
    hipLaunchKernelGGL(scale_by_kernel<__bf16>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (__bf16*)y, (const __bf16*)x, n, scale);
  else if (dtype == SR_DTYPE_F32)
    hipLaunchKernelGGL(scale_by_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (float*)y, (const float*)x, n, scale);
  else return -1;
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
// forward + loss-folded backward + Adam from ONE call: net->hr / loss_kind / loss_gscale / loss_part set by the caller;
// `flat` is updated in place, *loss_out = loss_scale * sum(loss partials)
extern "C" int sr_wdsr_net_train_step(const sr_wdsr_net_t* n, float* m, float* v, long n_params, const sr_adam_t* a,
                                      float loss_scale, float* loss_out, sr_stream_t stream) {
  if (!n || !n->hr || !m || !v || !a || n_params <= 0) return -2;
  int rc;
  const bool tail_train = net_step_fuses_tail(n);
  if ((rc = sr_wdsr_net_forward(n, SR_NET_SAVE_ACTS | (tail_train ? SR_NET_SKIP_TAIL : 0), stream))) return rc;
  // every parameter belongs to exactly one row of the weight-norm tables (the caller checks it: n_params == rows' elements),
  // so the Adam update rides on the weight-norm backward
  const FusedAdam fa{m, v, AdamArgs{a->w_lerp, a->beta2, a->one_minus_beta2, a->bc2_sqrt, a->eps, a->neg_step_size}, n->loss_part,
                     n->wgs_tail, loss_scale, loss_out};
  if ((rc = net_backward_part_impl(n, 0, stream, n->adam_in_wn_bwd ? &fa : nullptr, tail_train)) || n->adam_in_wn_bwd) return rc;
  return sr_adam_step(const_cast<float*>(n->flat), n->gflat, m, v, n_params, a, n->loss_part, n->wgs_tail, loss_scale, loss_out, stream);
}

// ------------------------------------------------------------------------------------------
// probes
// ------------------------------------------------------------------------------------------
__global__ void probe_mfma_bf16_kernel(const bf16x8* a, const bf16x8* b, float* out) {
  const int l = threadIdx.x;
  f32x16 acc = zero16();
  acc = mma16<__bf16>(a[l], b[l], acc);
#pragma unroll
  for (int i = 0; i < 16; ++i) out[l * 16 + i] = acc[i];
}
__global__ void probe_mfma_f32_kernel(const f32x8* a, const f32x8* b, float* out) {
  const int l = threadIdx.x;
  f32x16 acc = zero16();
  acc = mma16<float>(a[l], b[l], acc);
#pragma unroll
  for (int i = 0; i < 16; ++i) out[l * 16 + i] = acc[i];
}
__global__ void probe_tr_kernel(const __bf16* img, int n, const int* off, bf16x4* out) {
  __shared__ __attribute__((aligned(16))) __bf16 lds[8192];
  for (int i = threadIdx.x; i < n && i < 8192; i += 64) lds[i] = img[i];
  __syncthreads();
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  out[threadIdx.x] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(lds + off[threadIdx.x]));
}
__global__ void probe_copy_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, size_t n16) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = src[i];
}

extern "C" int sr_probe_mfma_bf16(const void* a, const void* b, float* out, sr_stream_t stream) {
  hipLaunchKernelGGL(probe_mfma_bf16_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const bf16x8*)a,
                     (const bf16x8*)b, out);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
extern "C" int sr_probe_mfma_f32(const float* a, const float* b, float* out, sr_stream_t stream) {
  hipLaunchKernelGGL(probe_mfma_f32_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const f32x8*)a,
                     (const f32x8*)b, out);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
extern "C" int sr_probe_tr_read(const void* img, int n, const int* off, void* out, sr_stream_t stream) {
  if (n > 8192) return -2;
  hipLaunchKernelGGL(probe_tr_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const __bf16*)img, n, off,
                     (bf16x4*)out);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
extern "C" int sr_probe_copy(const void* src, void* dst, size_t n_bytes, sr_stream_t stream) {
  if (n_bytes % 16) return -2;
  hipLaunchKernelGGL(probe_copy_kernel, dim3(256 * 8), dim3(256), 0, (hipStream_t)stream, (const u32x4*)src,
                     (u32x4*)dst, n_bytes / 16);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

// launch-floor probe: `reps` dependent launches of a kernel that does nothing but occupy `threads` threads and
// `lds_bytes` of LDS per workgroup (so one workgroup per CU when large) and write one word per workgroup
__global__ void probe_floor_kernel(unsigned* out) {
  extern __shared__ unsigned dyn_lds[];
  if (threadIdx.x == 0) {
    dyn_lds[0] = blockIdx.x;
    out[blockIdx.x + gridDim.x * blockIdx.y] = dyn_lds[0];
  }
}
extern "C" int sr_probe_launch_floor(void* out, int gx, int gy, int threads, int lds_bytes, int reps,
                                     sr_stream_t stream) {
  if (!out || gx <= 0 || gy <= 0 || threads <= 0 || threads > 1024 || lds_bytes < 4 || lds_bytes > 160 * 1024) return -2;
  if (hipFuncSetAttribute((const void*)probe_floor_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
    return -3;
  for (int i = 0; i < reps; ++i)
    hipLaunchKernelGGL(probe_floor_kernel, dim3(gx, gy), dim3(threads), lds_bytes, (hipStream_t)stream, (unsigned*)out);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

// same chain captured once in a hipGraph and replayed: separates the host's launch rate from the GPU's
// dependent-dispatch cost.  Synchronises; returns microseconds per kernel in *us_per_launch.
extern "C" int sr_probe_launch_floor_graph(void* out, int gx, int gy, int threads, int lds_bytes, int reps, int iters,
                                           float* us_per_launch, float* host_us_per_graph) {
  if (!out || !us_per_launch || gx <= 0 || gy <= 0 || threads <= 0 || threads > 1024 || lds_bytes < 4 ||
      lds_bytes > 160 * 1024 || reps <= 0 || iters <= 0)
    return -2;
  if (hipFuncSetAttribute((const void*)probe_floor_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
    return -3;
  hipStream_t s;
  hipGraph_t g;
  hipGraphExec_t ge;
  hipEvent_t e0, e1;
  int rc = -3;
  if (hipStreamCreate(&s) != hipSuccess) return -3;
  if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess) {
    for (int i = 0; i < reps; ++i)
      hipLaunchKernelGGL(probe_floor_kernel, dim3(gx, gy), dim3(threads), lds_bytes, s, (unsigned*)out);
    if (hipStreamEndCapture(s, &g) == hipSuccess) {
      if (hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) == hipSuccess) {
        hipEventCreate(&e0);
        hipEventCreate(&e1);
        hipGraphLaunch(ge, s);
        hipStreamSynchronize(s);
        hipEventRecord(e0, s);
        timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        for (int i = 0; i < iters; ++i) hipGraphLaunch(ge, s);
        clock_gettime(CLOCK_MONOTONIC, &t1);
        hipEventRecord(e1, s);
        hipStreamSynchronize(s);
        float ms = 0.f;
        hipEventElapsedTime(&ms, e0, e1);
        *us_per_launch = ms * 1e3f / ((float)reps * iters);
        if (host_us_per_graph) *host_us_per_graph = (float)(((t1.tv_sec - t0.tv_sec) * 1e9 + (t1.tv_nsec - t0.tv_nsec)) * 1e-3 / iters);
        hipEventDestroy(e0);
        hipEventDestroy(e1);
        hipGraphExecDestroy(ge);
        rc = 0;
      }
      hipGraphDestroy(g);
    }
  }
  hipStreamDestroy(s);
  return rc;
}

// debug: route the in-kernel time stamps of the diagnostic build to `buf` ([n_workgroups][16 waves][16 stamps][2] u64; NULL = off).
// Workgroups beyond n_workgroups do not stamp (a stamped launch with a larger grid must not write past the buffer).
// The product library carries no stamp code: there the call reports "unsupported".
extern "C" int sr_debug_set_stamps(void* buf, long n_workgroups) {
#ifdef SR_DEBUG_STAMPS
  if (buf && n_workgroups <= 0) return -2;
  unsigned long long* p = (unsigned long long*)buf;
  const unsigned long long n = buf ? (unsigned long long)n_workgroups : 0ull;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_sr_stamp_wgs), &n, sizeof(n)) != hipSuccess) return -3;
  return hipMemcpyToSymbol(HIP_SYMBOL(g_sr_stamps), &p, sizeof(p)) == hipSuccess ? 0 : -3;
#else
  (void)buf; (void)n_workgroups;
  return -1;
#endif
}

// ---- SPyNet's 7x7 convolutions (csrc/spynet_conv.h) ----
template <int CIN, int COUT, bool RELU, bool OUT_F32>
static int launch_conv7(const void* x, const void* w, const float* bias, void* y, int N, int H, int W, hipStream_t st) {
  typedef Conv7Cfg<CIN, COUT> K;
  const int tiles_x = (W + K::TW - 1) / K::TW, tiles_y = (H + K::TH - 1) / K::TH;
  hipLaunchKernelGGL((conv7_fwd_kernel<CIN, COUT, RELU, OUT_F32>), dim3(tiles_x * tiles_y, N), dim3(512), 0, st, (const __bf16*)x,
                     (const __bf16*)w, bias, y, H, W, tiles_x);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
extern "C" int sr_conv7_fwd(const void* x, const void* wpacked, const float* bias, void* y, int N, int H, int W, int CIN, int COUT,
                            int relu, int out_f32, sr_stream_t stream) {
  if (!x || !wpacked || !bias || !y || N <= 0 || H <= 0 || W <= 0 || N > 65535) return -2;
  hipStream_t st = (hipStream_t)stream;
  if (CIN == 8 && COUT == 32 && relu && !out_f32) return launch_conv7<8, 32, true, false>(x, wpacked, bias, y, N, H, W, st);
  if (CIN == 32 && COUT == 64 && relu && !out_f32) return launch_conv7<32, 64, true, false>(x, wpacked, bias, y, N, H, W, st);
  if (CIN == 64 && COUT == 32 && relu && !out_f32) return launch_conv7<64, 32, true, false>(x, wpacked, bias, y, N, H, W, st);
  if (CIN == 32 && COUT == 16 && relu && !out_f32) return launch_conv7<32, 16, true, false>(x, wpacked, bias, y, N, H, W, st);
  if (CIN == 16 && COUT == 2 && !relu && out_f32) return launch_conv7<16, 2, false, true>(x, wpacked, bias, y, N, H, W, st);
  return -1;
}

// backward-data of one layer: the forward kernel on the rotated, role-swapped table (packing.conv7_bwd_tables)
template <int CIN, int COUT, bool OUT_F32>
static int launch_conv7_bwd(const void* dy, const void* w, const void* act, void* dx, int N, int H, int W, hipStream_t st) {
  typedef Conv7Cfg<CIN, COUT> K;
  const int tiles_x = (W + K::TW - 1) / K::TW, tiles_y = (H + K::TH - 1) / K::TH;
  hipLaunchKernelGGL((conv7_fwd_kernel<CIN, COUT, false, OUT_F32, true>), dim3(tiles_x * tiles_y, N), dim3(512), 0, st,
                     (const __bf16*)dy, (const __bf16*)w, (const float*)nullptr, dx, H, W, tiles_x, (const __bf16*)act);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
static int conv7_bwd_data(const void* dy, const void* wt, const void* act, void* dx, int N, int H, int W, int CIN, int COUT,
                          hipStream_t st) {
  if (CIN == 8 && COUT == 32) return launch_conv7_bwd<32, 8, true>(dy, wt, nullptr, dx, N, H, W, st);
  if (CIN == 32 && COUT == 64) return launch_conv7_bwd<64, 32, false>(dy, wt, act, dx, N, H, W, st);
  if (CIN == 64 && COUT == 32) return launch_conv7_bwd<32, 64, false>(dy, wt, act, dx, N, H, W, st);
  if (CIN == 32 && COUT == 16) return launch_conv7_bwd<16, 32, false>(dy, wt, act, dx, N, H, W, st);
  if (CIN == 16 && COUT == 2) return launch_conv7_bwd<8, 16, false>(dy, wt, act, dx, N, H, W, st);
  return -1;
}
static bool conv7_layer(int CIN, int COUT) {
  return (CIN == 8 && COUT == 32) || (CIN == 32 && COUT == 64) || (CIN == 64 && COUT == 32) || (CIN == 32 && COUT == 16) ||
         (CIN == 16 && COUT == 2);
}
extern "C" int sr_conv7_bwd_data(const void* dy, const void* wpacked_t, const void* act, void* dx, int N, int H, int W, int CIN,
                                 int COUT, sr_stream_t stream) {
  if (!dy || !wpacked_t || !dx || N <= 0 || H <= 0 || W <= 0 || N > 65535) return -2;
  if (!conv7_layer(CIN, COUT)) return -1;
  if (CIN != 8 && !act) return -2;
  return conv7_bwd_data(dy, wpacked_t, act, dx, N, H, W, CIN, COUT, (hipStream_t)stream);
}

// weight gradient of one layer: partial slabs, then their sum in slab order into gflat = weight | bias (no float atomics)
template <int CA, int CB>
static int launch_conv7_wgrad(const void* dy, const void* x, float* partial, int wgs, int N, int H, int W, hipStream_t st) {
  typedef Conv7WgradCfg<CA, CB> C;
  const int tx = (W + C::TW - 1) / C::TW, ty = (H + C::TH - 1) / C::TH;
  hipLaunchKernelGGL((conv7_wgrad_kernel<CA, CB>), dim3(wgs, C::NG), dim3(512), 0, st, (const __bf16*)dy, (const __bf16*)x, partial,
                     N, H, W, tx, tx * ty);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
static long conv7_wgrad_slab(int CIN, int COUT) {                  // Conv7WgradCfg<max(COUT, 8), CIN>::SLAB
  const long nrt = (std::max(COUT, 8) + 31) / 32, nct = (CIN + 31) / 32;
  return nrt * (nct * 49 + 1) * 1024;
}
static int conv7_wgrad(const void* dy, const void* x, float* partial, int wgs, const int* sidx, const int* dst, float* gflat, int N,
                       int H, int W, int CIN, int COUT, hipStream_t st) {
  int rc;
  if (CIN == 8 && COUT == 32) rc = launch_conv7_wgrad<32, 8>(dy, x, partial, wgs, N, H, W, st);
  else if (CIN == 32 && COUT == 64) rc = launch_conv7_wgrad<64, 32>(dy, x, partial, wgs, N, H, W, st);
  else if (CIN == 64 && COUT == 32) rc = launch_conv7_wgrad<32, 64>(dy, x, partial, wgs, N, H, W, st);
  else if (CIN == 32 && COUT == 16) rc = launch_conv7_wgrad<16, 32>(dy, x, partial, wgs, N, H, W, st);
  else if (CIN == 16 && COUT == 2) rc = launch_conv7_wgrad<8, 16>(dy, x, partial, wgs, N, H, W, st);
  else return -1;
  if (rc) return rc;
  const int n = COUT * CIN * 49 + COUT;
  UnpackSegs us;
  us.nseg = 1;
  us.s[0] = UnpackSeg{partial, sidx, dst, 0, 0, conv7_wgrad_slab(CIN, COUT), wgs, n, 1, 0, 0};
  hipLaunchKernelGGL(unpack_all_kernel, dim3(unpack_blocks(n, wgs)), dim3(64 * UNPACK_Q), 0, st, gflat, us);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
extern "C" int sr_conv7_wgrad(const void* dy, const void* x, float* partial, int wgs, const int* sidx, const int* dst, float* gflat,
                              int N, int H, int W, int CIN, int COUT, sr_stream_t stream) {
  if (!dy || !x || !partial || !sidx || !dst || !gflat || wgs <= 0 || wgs > 65535 || N <= 0 || H <= 0 || W <= 0) return -2;
  if (!conv7_layer(CIN, COUT)) return -1;
  return conv7_wgrad(dy, x, partial, wgs, sidx, dst, gflat, N, H, W, CIN, COUT, (hipStream_t)stream);
}

// the whole backward of one BasicModule call: five weight gradients and five backward-data launches, last layer first
extern "C" int sr_conv7_module_bwd(const sr_conv7_module_bwd_t* m, int wgs, int N, int H, int W, sr_stream_t stream) {
  static const int LAYERS[5][2] = {{8, 32}, {32, 64}, {64, 32}, {32, 16}, {16, 2}};
  if (!m || !m->partial || !m->dx0 || wgs <= 0 || wgs > 65535 || N <= 0 || H <= 0 || W <= 0 || N > 65535) return -2;
  for (int l = 0; l < 5; ++l)
    if (!m->x[l] || !m->g[l] || !m->wpacked_t[l] || !m->sidx[l] || !m->dst[l] || !m->gflat[l]) return -2;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  for (int l = 4; l >= 0; --l) {                       // g[l]: the gradient at layer l's output; g[l - 1] = dx_l
    const int ci = LAYERS[l][0], co = LAYERS[l][1];
    if ((rc = conv7_wgrad(m->g[l], m->x[l], m->partial, wgs, m->sidx[l], m->dst[l], m->gflat[l], N, H, W, ci, co, st))) return rc;
    if ((rc = conv7_bwd_data(m->g[l], m->wpacked_t[l], m->x[l], l ? m->g[l - 1] : m->dx0, N, H, W, ci, co, st))) return rc;
  }
  return 0;
}

// ---- searched network (Result_Model): csrc/result_block.h ----
namespace {
template <typename T, int K, int CI, int COUT, int EP, int R>
int launch_rm_conv(const void* in, const void* res, void* out, float* hr, const void* wp, const float* bias, unsigned* mask, int N,
                   int H, int W, hipStream_t st) {
  typedef RmConvCfg<T, K, CI, COUT> C;
  const int tx = (W + C::TW - 1) / C::TW, ty = (H + C::TH - 1) / C::TH;
  hipLaunchKernelGGL((rm_conv_kernel<T, K, CI, COUT, EP, R>), dim3(tx * ty, N), dim3(256), 0, st, (const T*)in, (const T*)res,
                     (T*)out, hr, (const T*)wp, bias, (uint32_t*)mask, H, W, tx);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
#define SR_RM_DISPATCH_K(CALL, ...)                                                                        \
  if (K == 3) { CALL(3, __VA_ARGS__) } else if (K == 5) { CALL(5, __VA_ARGS__) } else if (K == 7) { CALL(7, __VA_ARGS__) } \
  else return -1;
#define SR_RM_DISPATCH_K57(CALL, ...)                                                                      \
  if (K == 5) { CALL(5, __VA_ARGS__) } else if (K == 7) { CALL(7, __VA_ARGS__) } else return -1;
#define SR_RM_DISPATCH_TF(CALL, DISP)                                                                      \
  if (dtype == SR_DTYPE_BF16 && F == 24) { DISP(CALL, __bf16, 24) }                                        \
  else if (dtype == SR_DTYPE_BF16 && F == 32) { DISP(CALL, __bf16, 32) }                                   \
  else if (dtype == SR_DTYPE_F32 && F == 24) { DISP(CALL, float, 24) }                                     \
  else if (dtype == SR_DTYPE_F32 && F == 32) { DISP(CALL, float, 32) }                                     \
  else return -1;
constexpr int rm_cp(int R) { return R == 2 ? 16 : R == 3 ? 32 : 48; }
}  // namespace

extern "C" int sr_rm_block_fwd(const void* x, void* y, unsigned* mask, const void* wp, const float* bias, int N, int H, int W, int F,
                               int K, int dtype, sr_stream_t stream) {
  if (!x || !y || !mask || !wp || !bias || N <= 0 || H <= 0 || W <= 0 || N > 65535) return -2;
  hipStream_t st = (hipStream_t)stream;
#define CALL(K_, T, F_) return launch_rm_conv<T, K_, F_, F_, RM_EP_BLOCK, 1>(x, x, y, nullptr, wp, bias, mask, N, H, W, st);
#define DISP(C_, T, F_) SR_RM_DISPATCH_K(C_, T, F_)
  SR_RM_DISPATCH_TF(CALL, DISP)
#undef DISP
#undef CALL
}

extern "C" int sr_rm_block_bwd_data(const void* dy, const unsigned* mask, void* dx, const void* wpt, int N, int H, int W, int F, int K,
                                    int dtype, sr_stream_t stream) {
  if (!dy || !mask || !dx || !wpt || N <= 0 || H <= 0 || W <= 0 || N > 65535) return -2;
  hipStream_t st = (hipStream_t)stream;
#define CALL(K_, T, F_) \
  return launch_rm_conv<T, K_, F_, F_, RM_EP_BWD, 1>(dy, dy, dx, nullptr, wpt, nullptr, (unsigned*)mask, N, H, W, st);
#define DISP(C_, T, F_) SR_RM_DISPATCH_K(C_, T, F_)
  SR_RM_DISPATCH_TF(CALL, DISP)
#undef DISP
#undef CALL
}

namespace {
template <typename T, int K, int CA, int CB, bool MASK>
int launch_rm_wgrad(const void* g, const unsigned* mask, const void* xin, float* partial, int wgs, int N, int H, int W,
                    hipStream_t st) {
  typedef RmWgradCfg<T, K, CA, CB> C;
  const int tx = (W + C::TW - 1) / C::TW, tpi = tx * ((H + C::TH - 1) / C::TH);
  hipLaunchKernelGGL((rm_wgrad_kernel<T, K, CA, CB, MASK>), dim3(wgs, C::NG), dim3(512), 0, st, (const T*)g, (const uint32_t*)mask,
                     (const T*)xin, partial, N, H, W, tx, tpi);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
}  // namespace

extern "C" int sr_rm_wgrad(const void* g, const unsigned* mask, const void* xin, float* partial, int wgs, int N, int H, int W, int CA,
                           int CB, int K, int dtype, sr_stream_t stream) {
  if (!g || !xin || !partial || wgs <= 0 || N <= 0 || H <= 0 || W <= 0) return -2;
  hipStream_t st = (hipStream_t)stream;
  const int F = CB;
  if (mask) {
    if (CA != CB) return -1;
#define CALL(K_, T, F_) return launch_rm_wgrad<T, K_, F_, F_, true>(g, mask, xin, partial, wgs, N, H, W, st);
#define DISP(C_, T, F_) SR_RM_DISPATCH_K(C_, T, F_)
    SR_RM_DISPATCH_TF(CALL, DISP)
#undef DISP
#undef CALL
  }
#define CALLA(K_, T, F_, CA_) return launch_rm_wgrad<T, K_, CA_, F_, false>(g, nullptr, xin, partial, wgs, N, H, W, st);
#define CALL(K_, T, F_) \
  if (CA == 16) { CALLA(K_, T, F_, 16) } else if (CA == 32) { CALLA(K_, T, F_, 32) } else if (CA == 48) { CALLA(K_, T, F_, 48) } \
  else return -1;
#define DISP(C_, T, F_) SR_RM_DISPATCH_K57(C_, T, F_)
  SR_RM_DISPATCH_TF(CALL, DISP)
#undef DISP
#undef CALL
#undef CALLA
}

extern "C" int sr_rm_tail_fwd(const void* feat, float* out, const void* wp, int N, int H, int W, int F, int R, int K, int dtype,
                              sr_stream_t stream) {
  if (!feat || !out || !wp || N <= 0 || H <= 0 || W <= 0 || N > 65535) return -2;
  hipStream_t st = (hipStream_t)stream;
#define CALLR(K_, T, F_, R_) return launch_rm_conv<T, K_, F_, 3 * R_ * R_, RM_EP_SHUF, R_>(feat, nullptr, nullptr, out, wp, nullptr, \
                                                                                         nullptr, N, H, W, st);
#define CALL(K_, T, F_) if (R == 2) { CALLR(K_, T, F_, 2) } else if (R == 3) { CALLR(K_, T, F_, 3) } \
  else if (R == 4) { CALLR(K_, T, F_, 4) } else return -1;
#define DISP(C_, T, F_) SR_RM_DISPATCH_K57(C_, T, F_)
  SR_RM_DISPATCH_TF(CALL, DISP)
#undef DISP
#undef CALL
#undef CALLR
}

extern "C" int sr_rm_unshuffle(const float* dout, void* dconv, int N, int H, int W, int R, int dtype, sr_stream_t stream) {
  if (!dout || !dconv || N <= 0 || H <= 0 || W <= 0) return -2;
  hipStream_t st = (hipStream_t)stream;
  const long total = (long)N * H * W * 48;
  const int blocks = (int)std::min<long>((total + 255) / 256, 4096);
#define CALLR(T, R_) { hipLaunchKernelGGL((rm_unshuffle_kernel<T, R_, rm_cp(R_)>), dim3(blocks), dim3(256), 0, st, dout, (T*)dconv, N, H, W); }
#define CALL(T) if (R == 2) CALLR(T, 2) else if (R == 3) CALLR(T, 3) else if (R == 4) CALLR(T, 4) else return -1;
  if (dtype == SR_DTYPE_BF16) { CALL(__bf16) } else if (dtype == SR_DTYPE_F32) { CALL(float) } else return -1;
#undef CALL
#undef CALLR
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

extern "C" int sr_rm_tail_bwd_data(const void* dconv, void* dfeat, const void* wpt, int N, int H, int W, int F, int R, int K,
                                   int dtype, sr_stream_t stream) {
  if (!dconv || !dfeat || !wpt || N <= 0 || H <= 0 || W <= 0 || N > 65535) return -2;
  hipStream_t st = (hipStream_t)stream;
#define CALLR(K_, T, F_, R_) return launch_rm_conv<T, K_, rm_cp(R_), F_, RM_EP_STORE, R_>(dconv, nullptr, dfeat, nullptr, wpt, \
                                                                                         nullptr, nullptr, N, H, W, st);
#define CALL(K_, T, F_) if (R == 2) { CALLR(K_, T, F_, 2) } else if (R == 3) { CALLR(K_, T, F_, 3) } \
  else if (R == 4) { CALLR(K_, T, F_, 4) } else return -1;
#define DISP(C_, T, F_) SR_RM_DISPATCH_K57(C_, T, F_)
  SR_RM_DISPATCH_TF(CALL, DISP)
#undef DISP
#undef CALL
#undef CALLR
}

// ------------------------------------------------------------------------------------------
// what the two video networks' drivers share
// ------------------------------------------------------------------------------------------
namespace {
// nb blocks over NF frames of H x W: within the kernels' reach?  (frames are grid.y.)  train: the training kernels also walk frames x
// tiles with an int; the smallest tile is the weight-gradient kernels' 16 x 16 / the upsampler's 8 x 16
bool clip_geometry_ok(int nb, long NF, int H, int W, int dtype, bool train) {
  if (NF > 65535 || H > 8192 || W > 8192 || nb > 1024 || (dtype != SR_DTYPE_BF16 && dtype != SR_DTYPE_F32)) return false;
  return !train || NF * ((W + 15) / 16) * ((H + 7) / 8) <= 2147483647L;
}

// One block y = conv2(ReLU(conv1(x))) + x backwards, 32 wide: dy -> dt through w2t, dW2 / db2 from (dy, t) into slab2; dt & mask (+ dy,
// the skip) -> dx through w1t, dW1 / db1 from (dt & mask, x) into slab1.  w1t, w2t: the transposed, flipped operands.
template <typename T>
int rm_block_bwd(const T* dy, T* dt, T* dx, const T* x, const T* t, const unsigned* mask, const T* w1t, const T* w2t, float* slab1,
                 float* slab2, int wgs, int N, int H, int W, hipStream_t st) {
  int rc;
  if ((rc = launch_rm_conv<T, 3, 32, 32, RM_EP_STORE, 1>(dy, nullptr, dt, nullptr, w2t, nullptr, nullptr, N, H, W, st))) return rc;
  if ((rc = launch_rm_wgrad<T, 3, 32, 32, false>(dy, nullptr, t, slab2, wgs, N, H, W, st))) return rc;
  if ((rc = launch_rm_conv<T, 3, 32, 32, RM_EP_BWD, 1>(dt, dy, dx, nullptr, w1t, nullptr, (unsigned*)mask, N, H, W, st))) return rc;
  return launch_rm_wgrad<T, 3, 32, 32, true>(dt, mask, x, slab1, wgs, N, H, W, st);
}
}  // namespace

// ------------------------------------------------------------------------------------------
// per-frame video network (models/single_image_model.py), inference: csrc/frame_net.h
// ------------------------------------------------------------------------------------------
namespace {
// the sized entry points' own arguments: four tables, 1 <= OH, OW <= SR_FN_MAX_OUT (the tables' and the kernels' int indices)
int fn_resize_check(const FnResize& rz) {
  if (!rz.ty || !rz.ly || !rz.tx || !rz.lx || rz.OH < 1 || rz.OW < 1) return -2;
  return rz.OH > SR_FN_MAX_OUT || rz.OW > SR_FN_MAX_OUT ? -1 : 0;
}

// rz: null = sr_fn_net_fwd, else the sized upsampler (SR_FN_WRITE_D is then not accepted)
int fn_net_fwd_impl(const float* frames, const void* blob, const long* conv_off, const void* head_blob, void* s0, void* s1, void* s2,
                    float* out, long out_is, int nb, int N, int H, int W, int dtype, int stages, const FnResize* rz, sr_stream_t stream) {
  if (!frames || !blob || !conv_off || !head_blob || !s0 || !s1 || !s2 || !out) return -2;
  if (nb < 0 || N <= 0 || H <= 0 || W <= 0 || stages <= 0 || stages >= (rz ? SR_FN_WRITE_D : 2 * SR_FN_WRITE_D)) return -2;
  if (rz && fn_resize_check(*rz) == -2) return -2;
  if (!clip_geometry_ok(nb, N, H, W, dtype, false) || (rz && fn_resize_check(*rz))) return -1;
  const bool write_d = (stages & SR_FN_WRITE_D) != 0;
  if ((stages & SR_FN_UP) && out_is < (rz ? 3L * rz->OH * rz->OW : write_d ? 3L * (4 * H + 1) * (4 * W + 1) : 48L * H * W)) return -2;
  hipStream_t st = (hipStream_t)stream;
  typedef FnCfg C;
  if (stages & SR_FN_ENCODER) {
    const int rc = sr_head_fwd(frames, s0, head_blob, 0.f, N, H, W, 32, dtype, stream);
    if (rc) return rc;
  }
  const int tiles_x = (W + C::TW - 1) / C::TW;
  const dim3 grid(tiles_x * ((H + C::TH - 1) / C::TH), N);
  const int utx = (W + C::UTW - 1) / C::UTW;
  const dim3 ugrid(utx * ((H + C::UTH - 1) / C::UTH), N);
  auto run = [&](auto tag) -> int {
    typedef decltype(tag) T;
    const T* const b = (const T*)blob;
    T* cur = (T*)s0;
    for (int i = 0; i < nb; ++i) {
      T* const dst = cur == (T*)s1 ? (T*)s2 : (T*)s1;
      if (stages & SR_FN_BLOCKS) {
        hipLaunchKernelGGL((fn_block_kernel<T, false>), grid, dim3(C::NT), 0, st, (const T*)cur, (const T*)nullptr, dst,
                           b + conv_off[2 * i], H, W, tiles_x);
        SR_HIP_CHECK_LAUNCH();
      }
      cur = dst;
    }
    T* const f = cur == (T*)s1 ? (T*)s2 : (T*)s1;
    if (stages & SR_FN_LAST) {
      hipLaunchKernelGGL((fn_block_kernel<T, true>), grid, dim3(C::NT), 0, st, (const T*)cur, (const T*)s0, f, b + conv_off[2 * nb], H,
                         W, tiles_x);
      SR_HIP_CHECK_LAUNCH();
    }
    if (stages & SR_FN_UP) {
      if (rz)
        hipLaunchKernelGGL((fn_up_sized_kernel<T>), ugrid, dim3(C::NT), 0, st, (const T*)f, b + conv_off[2 * nb + 1], out, out_is, H, W, utx,
                           *rz);
      else if (write_d)
        hipLaunchKernelGGL((fn_up_kernel<T, true>), ugrid, dim3(C::NT), 0, st, (const T*)f, b + conv_off[2 * nb + 1], out, out_is, H, W, utx);
      else
        hipLaunchKernelGGL((fn_up_kernel<T, false>), ugrid, dim3(C::NT), 0, st, (const T*)f, b + conv_off[2 * nb + 1], out, out_is, H, W, utx);
      SR_HIP_CHECK_LAUNCH();
    }
    return 0;
  };
  return dtype == SR_DTYPE_BF16 ? run(__bf16{}) : run(float{});
}
}  // namespace

extern "C" int sr_fn_net_fwd(const float* frames, const void* blob, const long* conv_off, const void* head_blob, void* s0, void* s1,
                             void* s2, float* out, long out_is, int nb, int N, int H, int W, int dtype, int stages,
                             sr_stream_t stream) {
  return fn_net_fwd_impl(frames, blob, conv_off, head_blob, s0, s1, s2, out, out_is, nb, N, H, W, dtype, stages, nullptr, stream);
}

extern "C" int sr_fn_net_fwd_sized(const float* frames, const void* blob, const long* conv_off, const void* head_blob, void* s0,
                                   void* s1, void* s2, float* out, long out_is, int OH, int OW, const int* ty, const float* ly,
                                   const int* tx, const float* lx, int nb, int N, int H, int W, int dtype, int stages,
                                   sr_stream_t stream) {
  const FnResize rz{ty, ly, tx, lx, OH, OW};
  return fn_net_fwd_impl(frames, blob, conv_off, head_blob, s0, s1, s2, out, out_is, nb, N, H, W, dtype, stages, &rz, stream);
}

// ------------------------------------------------------------------------------------------
// per-frame video network, the training route: csrc/frame_net.h (forward that saves), csrc/frame_net_bwd.h + csrc/result_block.h
// ------------------------------------------------------------------------------------------
namespace {
int fn_net_train_fwd_impl(const float* frames, const void* blob, const long* conv_off, const void* head_blob, void* acts, void* ts,
                          unsigned* masks, float* out, long out_is, int nb, int N, int H, int W, int dtype, int stages,
                          const FnResize* rz, sr_stream_t stream) {
  if (!frames || !blob || !conv_off || !head_blob || !acts || !out) return -2;
  if (nb < 0 || N <= 0 || H <= 0 || W <= 0 || stages <= 0 || stages > SR_FN_ALL || (nb > 0 && (!ts || !masks))) return -2;
  if (rz && fn_resize_check(*rz) == -2) return -2;
  if (!clip_geometry_ok(nb, N, H, W, dtype, true) || (rz && fn_resize_check(*rz))) return -1;
  if ((stages & SR_FN_UP) && out_is < (rz ? 3L * rz->OH * rz->OW : 48L * H * W)) return -2;
  hipStream_t st = (hipStream_t)stream;
  typedef FnCfg C;
  if (stages & SR_FN_ENCODER) {
    const int rc = sr_head_fwd(frames, acts, head_blob, 0.f, N, H, W, 32, dtype, stream);
    if (rc) return rc;
  }
  const int tiles_x = (W + C::TW - 1) / C::TW;
  const dim3 grid(tiles_x * ((H + C::TH - 1) / C::TH), N);
  const int utx = (W + C::UTW - 1) / C::UTW;
  const dim3 ugrid(utx * ((H + C::UTH - 1) / C::UTH), N);
  const size_t img = (size_t)N * H * W;
  auto run = [&](auto tag) -> int {
    typedef decltype(tag) T;
    const T* const b = (const T*)blob;
    T* const a = (T*)acts;
    if (stages & SR_FN_BLOCKS) {
      for (int i = 0; i < nb; ++i) {
        hipLaunchKernelGGL((fn_block_train_kernel<T>), grid, dim3(C::NT), 0, st, (const T*)(a + i * img * 32), a + (i + 1) * img * 32,
                           b + conv_off[2 * i], (T*)ts + i * img * 32, (uint32_t*)masks + i * img, H, W, tiles_x);
        SR_HIP_CHECK_LAUNCH();
      }
    }
    T* const f = a + (size_t)(nb + 1) * img * 32;
    if (stages & SR_FN_LAST) {
      hipLaunchKernelGGL((fn_block_kernel<T, true>), grid, dim3(C::NT), 0, st, (const T*)(a + nb * img * 32), (const T*)a, f,
                         b + conv_off[2 * nb], H, W, tiles_x);
      SR_HIP_CHECK_LAUNCH();
    }
    if (stages & SR_FN_UP) {
      if (rz)
        hipLaunchKernelGGL((fn_up_sized_kernel<T>), ugrid, dim3(C::NT), 0, st, (const T*)f, b + conv_off[2 * nb + 1], out, out_is, H, W, utx,
                           *rz);
      else
        hipLaunchKernelGGL((fn_up_kernel<T, false>), ugrid, dim3(C::NT), 0, st, (const T*)f, b + conv_off[2 * nb + 1], out, out_is, H, W, utx);
      SR_HIP_CHECK_LAUNCH();
    }
    return 0;
  };
  return dtype == SR_DTYPE_BF16 ? run(__bf16{}) : run(float{});
}
}  // namespace

extern "C" int sr_fn_net_train_fwd(const float* frames, const void* blob, const long* conv_off, const void* head_blob, void* acts,
                                   void* ts, unsigned* masks, float* out, long out_is, int nb, int N, int H, int W, int dtype,
                                   int stages, sr_stream_t stream) {
  return fn_net_train_fwd_impl(frames, blob, conv_off, head_blob, acts, ts, masks, out, out_is, nb, N, H, W, dtype, stages, nullptr, stream);
}

extern "C" int sr_fn_net_train_fwd_sized(const float* frames, const void* blob, const long* conv_off, const void* head_blob, void* acts,
                                         void* ts, unsigned* masks, float* out, long out_is, int OH, int OW, const int* ty,
                                         const float* ly, const int* tx, const float* lx, int nb, int N, int H, int W, int dtype,
                                         int stages, sr_stream_t stream) {
  const FnResize rz{ty, ly, tx, lx, OH, OW};
  return fn_net_train_fwd_impl(frames, blob, conv_off, head_blob, acts, ts, masks, out, out_is, nb, N, H, W, dtype, stages, &rz, stream);
}

namespace {
// loss_kind 0: g is d(loss)/d(out); 1 / 2: g is the network's output sr, hr the target, the gradient is formed in fn_up_bwd_kernel.
// rz: g (and hr) is (3, OH, OW) and the first stage is fn_up_bwd_sized_kernel, with the same loss kinds
int fn_net_bwd_impl(const float* frames, const float* g, const float* hr, int loss_kind, float gscale, float* loss_part, long g_is,
                    const void* bwd_blob, const void* acts, const void* ts, const unsigned* masks, void* gs, float* parts, int wgs,
                    float* grads, int C, int nb, int N, int H, int W, int dtype, int stages, sr_stream_t stream,
                    const FnResize* rz = nullptr) {
  if (!frames || !g || !bwd_blob || !acts || !gs || !parts || !grads) return -2;
  if (nb < 0 || N <= 0 || H <= 0 || W <= 0 || stages <= 0 || stages > SR_FN_BWD_ALL || C < 1 || C > 32 || wgs < 1 || wgs > 1024) return -2;
  if (nb > 0 && (!ts || !masks)) return -2;
  if (rz && fn_resize_check(*rz) == -2) return -2;
  if (!clip_geometry_ok(nb, N, H, W, dtype, true) || (rz && fn_resize_check(*rz))) return -1;
  if (g_is < (rz ? 3L * rz->OH * rz->OW : 48L * H * W)) return -2;
  hipStream_t st = (hipStream_t)stream;
  typedef FnBwdCfg B;
  const size_t img = (size_t)N * H * W;
  const int nconv = 2 * nb + 1;
  int up_wgs = 0;
  auto run = [&](auto tag) -> int {
    typedef decltype(tag) T;
    const T* const wb = (const T*)bwd_blob;
    const T* const a = (const T*)acts;
    T* const G = (T*)gs;
    T* const df = G;
    T* const dt = G + 2 * img * 32;
    auto conv_slab = [&](int j) { return parts + (size_t)j * wgs * B::CONV_SLAB; };
    int rc;
    if (stages & SR_FN_BWD_UP) {
      const int tiles_x = (W + B::TW - 1) / B::TW, tiles = tiles_x * ((H + B::TH - 1) / B::TH);
      up_wgs = (int)std::min<long>((long)N * tiles, wgs);
      if (rz && loss_kind == 0) {
        hipLaunchKernelGGL((fn_up_bwd_sized_kernel<T>), dim3(up_wgs), dim3(B::NT), 0, st, a + (size_t)(nb + 1) * img * 32, g, g_is,
                           wb + (size_t)nconv * B::CONV_ELEMS, df, conv_slab(nconv), N, H, W, tiles_x, tiles, *rz);
      } else if (rz && loss_kind == 1) {
        hipLaunchKernelGGL((fn_up_bwd_sized_kernel<T, 1>), dim3(up_wgs), dim3(B::NT), 0, st, a + (size_t)(nb + 1) * img * 32, g, g_is,
                           wb + (size_t)nconv * B::CONV_ELEMS, df, conv_slab(nconv), N, H, W, tiles_x, tiles, *rz, LossIn{hr, gscale},
                           loss_part);
      } else if (rz) {
        hipLaunchKernelGGL((fn_up_bwd_sized_kernel<T, 2>), dim3(up_wgs), dim3(B::NT), 0, st, a + (size_t)(nb + 1) * img * 32, g, g_is,
                           wb + (size_t)nconv * B::CONV_ELEMS, df, conv_slab(nconv), N, H, W, tiles_x, tiles, *rz, LossIn{hr, gscale},
                           loss_part);
      } else if (loss_kind == 0) {
        hipLaunchKernelGGL((fn_up_bwd_kernel<T>), dim3(up_wgs), dim3(B::NT), 0, st, a + (size_t)(nb + 1) * img * 32, g, g_is,
                           wb + (size_t)nconv * B::CONV_ELEMS, df, conv_slab(nconv), N, H, W, tiles_x, tiles);
      } else if (loss_kind == 1) {
        hipLaunchKernelGGL((fn_up_bwd_kernel<T, 1>), dim3(up_wgs), dim3(B::NT), 0, st, a + (size_t)(nb + 1) * img * 32, g, g_is,
                           wb + (size_t)nconv * B::CONV_ELEMS, df, conv_slab(nconv), N, H, W, tiles_x, tiles, LossIn{hr, gscale}, loss_part);
      } else {
        hipLaunchKernelGGL((fn_up_bwd_kernel<T, 2>), dim3(up_wgs), dim3(B::NT), 0, st, a + (size_t)(nb + 1) * img * 32, g, g_is,
                           wb + (size_t)nconv * B::CONV_ELEMS, df, conv_slab(nconv), N, H, W, tiles_x, tiles, LossIn{hr, gscale}, loss_part);
      }
      SR_HIP_CHECK_LAUNCH();
    }
    T* cur = G + img * 32;                                 // dz, then every block's dx in gs[3], gs[1], gs[3], ..
    if (stages & SR_FN_BWD_LAST) {
      if ((rc = launch_rm_conv<T, 3, 32, 32, RM_EP_STORE, 1>(df, nullptr, cur, nullptr, wb + (size_t)2 * nb * B::CONV_ELEMS, nullptr,
                                                              nullptr, N, H, W, st)))
        return rc;
      if ((rc = launch_rm_wgrad<T, 3, 32, 32, false>(df, nullptr, a + (size_t)nb * img * 32, conv_slab(2 * nb), wgs, N, H, W, st))) return rc;
    }
    for (int i = nb - 1; i >= 0; --i) {
      T* const dx = cur == G + img * 32 ? G + 3 * img * 32 : G + img * 32;
      if (stages & SR_FN_BWD_BLOCKS) {
        const T* const w = wb + (size_t)2 * i * B::CONV_ELEMS;
        if ((rc = rm_block_bwd<T>(cur, dt, dx, a + (size_t)i * img * 32, (const T*)ts + i * img * 32, masks + i * img, w, w + B::CONV_ELEMS,
                                  conv_slab(2 * i), conv_slab(2 * i + 1), wgs, N, H, W, st)))
          return rc;
      }
      cur = dx;
    }
    if (stages & SR_FN_BWD_ENCODER) {                      // de = dx_0 + df into gs[2] (dt is dead)
      const size_t n_vec = img * 8;
      hipLaunchKernelGGL((fn_add_kernel<T>), dim3((unsigned)std::min<size_t>((n_vec + 255) / 256, 4096)), dim3(256), 0, st, (const T*)cur,
                         (const T*)df, dt, n_vec);
      SR_HIP_CHECK_LAUNCH();
      if ((rc = sr_head_wgrad(dt, frames, 0.f, conv_slab(nconv) + (size_t)wgs * B::SLAB, wgs, N, H, W, 32, dtype, stream))) return rc;
    }
    return 0;
  };
  const int rc = dtype == SR_DTYPE_BF16 ? run(__bf16{}) : run(float{});
  if (rc) return rc;
  const int per = std::max(9 * C * C + C, 75 * C + 3);
  hipLaunchKernelGGL(fn_reduce_kernel, dim3((per + 255) / 256, nconv + 2), dim3(256), 0, st, (const float*)parts, grads, C, nb, wgs,
                     up_wgs, stages & SR_FN_BWD_BLOCKS, stages & SR_FN_BWD_LAST, stages & SR_FN_BWD_UP, stages & SR_FN_BWD_ENCODER);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
}  // namespace

extern "C" int sr_fn_net_bwd(const float* frames, const float* g, long g_is, const void* bwd_blob, const void* acts, const void* ts,
                             const unsigned* masks, void* gs, float* parts, int wgs, float* grads, int C, int nb, int N, int H, int W,
                             int dtype, int stages, sr_stream_t stream) {
  return fn_net_bwd_impl(frames, g, nullptr, 0, 0.f, nullptr, g_is, bwd_blob, acts, ts, masks, gs, parts, wgs, grads, C, nb, N, H, W, dtype,
                         stages, stream);
}

extern "C" int sr_fn_net_bwd_sized(const float* frames, const float* g, long g_is, int OH, int OW, const int* ty, const float* ly,
                                   const int* tx, const float* lx, const void* bwd_blob, const void* acts, const void* ts,
                                   const unsigned* masks, void* gs, float* parts, int wgs, float* grads, int C, int nb, int N, int H,
                                   int W, int dtype, int stages, sr_stream_t stream) {
  const FnResize rz{ty, ly, tx, lx, OH, OW};
  return fn_net_bwd_impl(frames, g, nullptr, 0, 0.f, nullptr, g_is, bwd_blob, acts, ts, masks, gs, parts, wgs, grads, C, nb, N, H, W, dtype,
                         stages, stream, &rz);
}

extern "C" int sr_fn_net_bwd_loss(const float* frames, const float* sr, const float* hr, int loss_kind, float gscale, float* loss_part,
                                  long g_is, const void* bwd_blob, const void* acts, const void* ts, const unsigned* masks, void* gs,
                                  float* parts, int wgs, float* grads, int C, int nb, int N, int H, int W, int dtype, int stages,
                                  sr_stream_t stream) {
  if (!hr || !loss_part || (loss_kind != 1 && loss_kind != 2) || stages <= 0 || !(stages & SR_FN_BWD_UP)) return -2;
  return fn_net_bwd_impl(frames, sr, hr, loss_kind, gscale, loss_part, g_is, bwd_blob, acts, ts, masks, gs, parts, wgs, grads, C, nb, N, H,
                         W, dtype, stages, stream);
}

extern "C" int sr_fn_net_bwd_loss_sized(const float* frames, const float* sr, const float* hr, int loss_kind, float gscale,
                                        float* loss_part, long g_is, int OH, int OW, const int* ty, const float* ly, const int* tx,
                                        const float* lx, const void* bwd_blob, const void* acts, const void* ts, const unsigned* masks,
                                        void* gs, float* parts, int wgs, float* grads, int C, int nb, int N, int H, int W, int dtype,
                                        int stages, sr_stream_t stream) {
  if (!hr || !loss_part || (loss_kind != 1 && loss_kind != 2) || stages <= 0 || !(stages & SR_FN_BWD_UP)) return -2;
  const FnResize rz{ty, ly, tx, lx, OH, OW};
  return fn_net_bwd_impl(frames, sr, hr, loss_kind, gscale, loss_part, g_is, bwd_blob, acts, ts, masks, gs, parts, wgs, grads, C, nb, N, H,
                         W, dtype, stages, stream, &rz);
}

// ------------------------------------------------------------------------------------------
// multi-frame video network (models/naive_multi_model_easy.py), inference: csrc/multi_frame.h
// ------------------------------------------------------------------------------------------
extern "C" int sr_mf_net_fwd(const float* frames, const float* flows, const void* blob, const void* head_blob, void* s0, void* s1,
                             void* s2, float* out, int nb, int B, int N, int H, int W, int dtype, int stages, sr_stream_t stream) {
  if (!frames || !blob || !head_blob || !s0 || !s1 || !s2 || !out) return -2;
  if (nb < 1 || B <= 0 || N <= 0 || H <= 0 || W <= 0 || stages <= 0 || stages > SR_MF_ALL || (N > 1 && !flows)) return -2;
  if (B > 65535 || N > 65535 || !clip_geometry_ok(nb, (long)B * N, H, W, dtype, false)) return -1;
  hipStream_t st = (hipStream_t)stream;
  typedef FnCfg C;
  const int frames_n = B * N;
  if (stages & SR_MF_ENCODER) {
    const int rc = sr_head_fwd(frames, s0, head_blob, 0.f, frames_n, H, W, 32, dtype, stream);
    if (rc) return rc;
  }
  const int tiles_x = (W + C::TW - 1) / C::TW;
  const dim3 grid(tiles_x * ((H + C::TH - 1) / C::TH), frames_n);
  auto run = [&](auto tag) -> int {
    typedef decltype(tag) T;
    const T* const b = (const T*)blob;
    if (stages & SR_MF_FIRST) {
      hipLaunchKernelGGL((mf_first_kernel<T>), grid, dim3(C::NT), 0, st, (const T*)s0, flows, (T*)s1, b, H, W, tiles_x, N);
      SR_HIP_CHECK_LAUNCH();
    }
    T* cur = (T*)s1;
    for (int i = 1; i < nb; ++i) {
      T* const dst = cur == (T*)s1 ? (T*)s2 : (T*)s1;
      if (stages & SR_MF_BLOCKS) {
        hipLaunchKernelGGL((fn_block_kernel<T, false>), grid, dim3(C::NT), 0, st, (const T*)cur, (const T*)nullptr, dst,
                           b + MfCfg::FIRST_ELEMS + (size_t)(i - 1) * 2 * C::CONV_ELEMS, H, W, tiles_x);
        SR_HIP_CHECK_LAUNCH();
      }
      cur = dst;
    }
    if (stages & SR_MF_TAIL) {
      hipLaunchKernelGGL((mf_tail_kernel<T>), grid, dim3(C::NT), 0, st, (const T*)cur, frames, out,
                         b + MfCfg::FIRST_ELEMS + (size_t)(nb - 1) * 2 * C::CONV_ELEMS, H, W, tiles_x);
      SR_HIP_CHECK_LAUNCH();
    }
    return 0;
  };
  return dtype == SR_DTYPE_BF16 ? run(__bf16{}) : run(float{});
}

// ------------------------------------------------------------------------------------------
// multi-frame video network, the training route: csrc/multi_frame.h (forward that saves), csrc/multi_frame_bwd.h + csrc/result_block.h
// ------------------------------------------------------------------------------------------
extern "C" int sr_mf_net_train_fwd(const float* frames, const float* flows, const void* blob, const void* head_blob, void* acts, void* ts,
                                   unsigned* masks, void* wf, float* out, int nb, int B, int N, int H, int W, int dtype, int stages,
                                   sr_stream_t stream) {
  if (!frames || !blob || !head_blob || !acts || !ts || !masks || !wf || !out) return -2;
  if (nb < 1 || B <= 0 || N <= 0 || H <= 0 || W <= 0 || stages <= 0 || stages > SR_MF_ALL || (N > 1 && !flows)) return -2;
  if (B > 65535 || N > 65535 || !clip_geometry_ok(nb, (long)B * N, H, W, dtype, true)) return -1;
  hipStream_t st = (hipStream_t)stream;
  typedef FnCfg C;
  const int frames_n = B * N;
  if (stages & SR_MF_ENCODER) {
    const int rc = sr_head_fwd(frames, acts, head_blob, 0.f, frames_n, H, W, 32, dtype, stream);
    if (rc) return rc;
  }
  const int tiles_x = (W + C::TW - 1) / C::TW;
  const dim3 grid(tiles_x * ((H + C::TH - 1) / C::TH), frames_n);
  const size_t img = (size_t)frames_n * H * W;
  auto run = [&](auto tag) -> int {
    typedef decltype(tag) T;
    const T* const b = (const T*)blob;
    T* const a = (T*)acts;
    if (stages & SR_MF_FIRST) {
      hipLaunchKernelGGL((mf_first_train_kernel<T>), grid, dim3(C::NT), 0, st, (const T*)a, flows, a + img * 32, b, (T*)ts,
                         (uint32_t*)masks, (T*)wf, (T*)wf + img * 32, H, W, tiles_x, N);
      SR_HIP_CHECK_LAUNCH();
    }
    if (stages & SR_MF_BLOCKS) {
      for (int i = 1; i < nb; ++i) {
        hipLaunchKernelGGL((fn_block_train_kernel<T>), grid, dim3(C::NT), 0, st, (const T*)(a + i * img * 32), a + (i + 1) * img * 32,
                           b + MfCfg::FIRST_ELEMS + (size_t)(i - 1) * 2 * C::CONV_ELEMS, (T*)ts + i * img * 32,
                           (uint32_t*)masks + i * img, H, W, tiles_x);
        SR_HIP_CHECK_LAUNCH();
      }
    }
    if (stages & SR_MF_TAIL) {
      hipLaunchKernelGGL((mf_tail_kernel<T>), grid, dim3(C::NT), 0, st, (const T*)(a + nb * img * 32), frames, out,
                         b + MfCfg::FIRST_ELEMS + (size_t)(nb - 1) * 2 * C::CONV_ELEMS, H, W, tiles_x);
      SR_HIP_CHECK_LAUNCH();
    }
    return 0;
  };
  return dtype == SR_DTYPE_BF16 ? run(__bf16{}) : run(float{});
}

namespace {
// loss_kind 0: g is d(loss)/d(out); 1 / 2: g is the network's output sr, hr the target, dD comes from mf_dd_loss_kernel
int mf_net_bwd_impl(const float* frames, const float* flows, const float* flow_bound, const float* g, const float* hr, int loss_kind,
                    float gscale, float* loss_part, const void* bwd_blob, const void* acts, const void* ts, const unsigned* masks,
                    const void* wf, void* gs, float* parts, int wgs, float* grads, int C, int nb, int B, int N, int H, int W, int dtype,
                    int stages, sr_stream_t stream) {
  if (!frames || !g || !bwd_blob || !acts || !ts || !masks || !wf || !gs || !parts || !grads) return -2;
  if (nb < 1 || B <= 0 || N <= 0 || H <= 0 || W <= 0 || stages <= 0 || stages > SR_MF_BWD_ALL || C < 1 || C > 32 || wgs < 1 || wgs > 1024)
    return -2;
  if (N > 1 && (!flows || !flow_bound)) return -2;
  if (B > 65535 || N > 65535 || !clip_geometry_ok(nb, (long)B * N, H, W, dtype, true)) return -1;
  hipStream_t st = (hipStream_t)stream;
  typedef MfBwdCfg M;
  const int NF = B * N;
  const size_t img = (size_t)NF * H * W;
  auto run = [&](auto tag) -> int {
    typedef decltype(tag) T;
    const T* const wb = (const T*)bwd_blob;
    const T* const a = (const T*)acts;
    const T* const tsv = (const T*)ts;
    T* const G = (T*)gs;
    T* const dt = G + 2 * img * 32;
    T* const dwarp = G + 3 * img * 32;
    T* const dD = G + 4 * img * 32;                          // [frame][H][W][48]
    auto slab = [&](int j) { return parts + (size_t)j * wgs * M::CONV_SLAB; };
    int rc;
    if (stages & SR_MF_BWD_TAIL) {
      if (loss_kind == 0) {
        const long total = (long)img * 48;
        hipLaunchKernelGGL((rm_unshuffle_kernel<T, 4, 48>), dim3((unsigned)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0, st, g,
                           dD, NF, H, W);
      } else {
        typedef MfLossCfg LC;
        const int ltx = (W + LC::TW - 1) / LC::TW, ltiles = ltx * ((H + LC::TH - 1) / LC::TH);
        const dim3 lgrid((unsigned)std::min<long>((long)NF * ltiles, wgs));
        if (loss_kind == 1)
          hipLaunchKernelGGL((mf_dd_loss_kernel<T, 1>), lgrid, dim3(LC::NT), 0, st, g, hr, gscale, dD, loss_part, NF, H, W, ltx, ltiles);
        else
          hipLaunchKernelGGL((mf_dd_loss_kernel<T, 2>), lgrid, dim3(LC::NT), 0, st, g, hr, gscale, dD, loss_part, NF, H, W, ltx, ltiles);
      }
      SR_HIP_CHECK_LAUNCH();
      if ((rc = launch_rm_conv<T, 3, 48, 32, RM_EP_STORE, 1>(dD, nullptr, G, nullptr, wb + M::dec_off(nb), nullptr, nullptr, NF, H, W, st)))
        return rc;
      if ((rc = launch_rm_wgrad<T, 3, 48, 32, false>(dD, nullptr, a + (size_t)nb * img * 32, slab(2 * nb + 2), wgs, NF, H, W, st))) return rc;
    }
    T* cur = G;                                              // block i's dy; its dx goes to the other of gs[0], gs[1]
    for (int i = nb - 1; i >= 1; --i) {
      T* const dx = cur == G ? G + img * 32 : G;
      if (stages & SR_MF_BWD_BLOCKS) {
        const T* const w = wb + M::block_off(i);
        if ((rc = rm_block_bwd<T>(cur, dt, dx, a + (size_t)i * img * 32, tsv + i * img * 32, masks + i * img, w, w + M::CONV_ELEMS,
                                  slab(2 * i), slab(2 * i + 1), wgs, NF, H, W, st)))
          return rc;
      }
      cur = dx;
    }
    T* const direct = cur == G ? G + img * 32 : G;           // de_direct
    if (stages & SR_MF_BWD_FIRST) {
      const T* const wfv = (const T*)wf;
      if ((rc = launch_rm_conv<T, 3, 32, 32, RM_EP_STORE, 1>(cur, nullptr, dt, nullptr, wb + 2 * M::CONV_ELEMS, nullptr, nullptr, NF, H, W, st)))
        return rc;
      if ((rc = launch_rm_wgrad<T, 3, 32, 32, false>(cur, nullptr, tsv, slab(1), wgs, NF, H, W, st))) return rc;
      if ((rc = launch_rm_conv<T, 3, 32, 32, RM_EP_BWD, 1>(dt, cur, direct, nullptr, wb, nullptr, (unsigned*)masks, NF, H, W, st))) return rc;
      if ((rc = launch_rm_conv<T, 3, 32, 32, RM_EP_MSTORE, 1>(dt, nullptr, dwarp, nullptr, wb + M::CONV_ELEMS, nullptr, (unsigned*)masks, NF, H,
                                                               W, st)))
        return rc;
      if ((rc = launch_rm_wgrad<T, 3, 32, 32, true>(dt, masks, a, slab(0), wgs, NF, H, W, st))) return rc;
      if ((rc = launch_rm_wgrad<T, 3, 32, 32, true>(dt, masks, wfv, slab(2 * nb), wgs, NF, H, W, st))) return rc;
      if ((rc = launch_rm_wgrad<T, 3, 32, 32, true>(dt, masks, wfv + img * 32, slab(2 * nb + 1), wgs, NF, H, W, st))) return rc;
    }
    if (stages & SR_MF_BWD_WARP) {                           // de into gs[2] (dt is dead)
      const int tx = (W + M::TS - 1) / M::TS;
      hipLaunchKernelGGL((mf_warp_bwd_kernel<T>), dim3(tx * ((H + M::TS - 1) / M::TS), NF), dim3(256), 0, st, (const T*)direct,
                         (const T*)dwarp, flows, flow_bound, dt, H, W, tx, N);
      SR_HIP_CHECK_LAUNCH();
    }
    if (stages & SR_MF_BWD_ENCODER) {
      if ((rc = sr_head_wgrad(dt, frames, 0.f, slab(2 * nb + 3), wgs, NF, H, W, 32, dtype, stream))) return rc;
    }
    return 0;
  };
  const int rc = dtype == SR_DTYPE_BF16 ? run(__bf16{}) : run(float{});
  if (rc) return rc;
  const int per = std::max(9 * C * (2 * C + 2) + C, 48 * 9 * C + 48);
  hipLaunchKernelGGL(mf_reduce_kernel, dim3((per + 255) / 256, 2 * nb + 2), dim3(256), 0, st, (const float*)parts, grads, C, nb, wgs,
                     stages & SR_MF_BWD_TAIL, stages & SR_MF_BWD_BLOCKS, stages & SR_MF_BWD_FIRST, stages & SR_MF_BWD_ENCODER);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}
}  // namespace

extern "C" int sr_mf_net_bwd(const float* frames, const float* flows, const float* flow_bound, const float* g, const void* bwd_blob,
                             const void* acts, const void* ts, const unsigned* masks, const void* wf, void* gs, float* parts, int wgs,
                             float* grads, int C, int nb, int B, int N, int H, int W, int dtype, int stages, sr_stream_t stream) {
  return mf_net_bwd_impl(frames, flows, flow_bound, g, nullptr, 0, 0.f, nullptr, bwd_blob, acts, ts, masks, wf, gs, parts, wgs, grads, C,
                         nb, B, N, H, W, dtype, stages, stream);
}

extern "C" int sr_mf_net_bwd_loss(const float* frames, const float* flows, const float* flow_bound, const float* sr, const float* hr,
                                  int loss_kind, float gscale, float* loss_part, const void* bwd_blob, const void* acts, const void* ts,
                                  const unsigned* masks, const void* wf, void* gs, float* parts, int wgs, float* grads, int C, int nb,
                                  int B, int N, int H, int W, int dtype, int stages, sr_stream_t stream) {
  if (!hr || !loss_part || (loss_kind != 1 && loss_kind != 2) || stages <= 0 || !(stages & SR_MF_BWD_TAIL)) return -2;
  return mf_net_bwd_impl(frames, flows, flow_bound, sr, hr, loss_kind, gscale, loss_part, bwd_blob, acts, ts, masks, wf, gs, parts, wgs,
                         grads, C, nb, B, N, H, W, dtype, stages, stream);
}

// ------------------------------------------------------------------------------------------
// the video networks' one-call training step: csrc/clip_param_step.h around the two networks' training entry points
// ------------------------------------------------------------------------------------------
static_assert(SR_CLIP_STEP_CAP == CLIP_STEP_CAP, "sr_hotpath.h and clip_param_step.h disagree");
namespace {
long clip_param_n(const sr_clip_param_t& p) { return p.p1 ? (long)p.rows * p.len : (long)p.len; }
int clip_param_blocks(const sr_clip_param_t& p) { return p.p1 ? (p.rows + 3) / 4 : (p.len + CLIP_STEP_CHUNK - 1) / CLIP_STEP_CHUNK; }

// everything the three launches index with, checked before the first of them
int clip_step_check(const sr_clip_step_t* s, long grads_n, int dtype) {
  if (!s || !s->params || s->n_params < 1 || !s->src || !s->inv || !s->adam || !s->loss_out || s->src_n < 1) return -2;
  if (dtype != SR_DTYPE_BF16 && dtype != SR_DTYPE_F32) return -1;
  long inv_rows = 0;
  for (int i = 0; i < s->n_params; ++i) {
    const sr_clip_param_t& p = s->params[i];
    if (!p.p0 || !p.m0 || !p.v0 || p.len < 1 || p.rows < 0 || p.src_off < 0 || p.grad_off < 0) return -2;
    if (p.p1 && (!p.m1 || !p.v1 || p.rows < 1)) return -2;
    const long n = clip_param_n(p);
    if (n > 2147483647L || p.src_off + n > s->src_n || p.grad_off + n > grads_n) return -2;
    if (p.p1) inv_rows += p.rows;
  }
  if (inv_rows > s->inv_n) return -2;
  for (int j = 0; j < 3; ++j)
    if (!s->idx[j] || !s->blob[j] || s->n_idx[j] < 1 || ((uintptr_t)s->blob[j] & 15)) return -2;
  return 0;
}

// weight norm + gather into s->src (ceil(n_params / CLIP_STEP_CAP) launches), then the three blobs (one launch)
// aten_order: the weight norm in torch._weight_norm's arithmetic (clip_wn_fwd_aten_kernel)
int clip_step_prologue(const sr_clip_step_t* s, int dtype, hipStream_t st, bool aten_order = false) {
  long inv_at = 0;
  for (int first = 0; first < s->n_params; first += CLIP_STEP_CAP) {
    const int count = std::min(CLIP_STEP_CAP, s->n_params - first);
    ClipWnTable t;
    int blocks = 0;
    for (int i = 0; i < CLIP_STEP_CAP; ++i) {
      if (i >= count) { t.row[i] = ClipWnRow{nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0}; continue; }
      const sr_clip_param_t& p = s->params[first + i];
      t.row[i] = p.p1 ? ClipWnRow{p.p0, p.p1, s->src + p.src_off, s->inv + inv_at, p.rows, p.len, blocks, 0}
                      : ClipWnRow{nullptr, p.p0, s->src + p.src_off, nullptr, 0, p.len, blocks, 0};
      if (p.p1) inv_at += p.rows;
      blocks += clip_param_blocks(p);
    }
    t.count = count;
    t.pad = 0;
    if (aten_order)
      hipLaunchKernelGGL(clip_wn_fwd_aten_kernel, dim3((unsigned)blocks), dim3(256), 0, st, t);
    else
      hipLaunchKernelGGL(clip_wn_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, st, t);
    SR_HIP_CHECK_LAUNCH();
  }
  ClipPackTable pt;
  long blocks = 0;
  for (int j = 0; j < CLIP_PACK_JOBS; ++j) {
    pt.row[j] = ClipPackJob{s->idx[j], s->blob[j], s->n_idx[j], (int)blocks, 0};
    blocks += (s->n_idx[j] + CLIP_PACK_CHUNK - 1) / CLIP_PACK_CHUNK;
  }
  if (blocks > 2147483647L) return -1;
  pt.count = CLIP_PACK_JOBS;
  pt.pad = 0;
  if (dtype == SR_DTYPE_BF16)
    hipLaunchKernelGGL(clip_pack_kernel<__bf16>, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)s->src, pt);
  else
    hipLaunchKernelGGL(clip_pack_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)s->src, pt);
  SR_HIP_CHECK_LAUNCH();
  return 0;
}

// weight-norm backward + Adam over every row; the last launch folds the loss: *loss_out = loss_weight / numel x sum(loss_part)
int clip_step_epilogue(const sr_clip_step_t* s, const float* grads, const float* loss_part, int n_loss, long numel, hipStream_t st) {
  const sr_adam_t* a = s->adam;
  long inv_at = 0;
  for (int first = 0; first < s->n_params; first += CLIP_STEP_CAP) {
    const int count = std::min(CLIP_STEP_CAP, s->n_params - first);
    const bool last = first + count == s->n_params;
    ClipStepTable t;
    int blocks = 0;
    for (int i = 0; i < CLIP_STEP_CAP; ++i) {
      if (i >= count) { t.row[i] = ClipStepRow{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0}; continue; }
      const sr_clip_param_t& p = s->params[first + i];
      t.row[i] = ClipStepRow{p.p0, p.p1, p.m0, p.v0, p.m1, p.v1, grads + p.grad_off, p.p1 ? s->inv + inv_at : nullptr,
                             p.rows, p.len, blocks, 0};
      if (p.p1) inv_at += p.rows;
      blocks += clip_param_blocks(p);
    }
    t.a = AdamArgs{a->w_lerp, a->beta2, a->one_minus_beta2, a->bc2_sqrt, a->eps, a->neg_step_size};
    t.gscale = s->loss_weight;
    t.loss_scale = (float)((double)s->loss_weight / (double)numel);
    t.loss_part = loss_part;
    t.loss_out = last ? s->loss_out : nullptr;
    t.n_loss = n_loss;
    t.count = count;
    hipLaunchKernelGGL(clip_wn_bwd_adam_kernel, dim3((unsigned)(blocks + (last ? 1 : 0))), dim3(256), 0, st, t);
    SR_HIP_CHECK_LAUNCH();
  }
  return 0;
}
}  // namespace

namespace {
// rz: null = sr_fn_net_train_step, else the sized forward and folded backward; every check precedes the first launch
int fn_net_train_step_impl(const sr_clip_step_t* step, const float* frames, const float* hr, int loss_kind, const long* conv_off,
                           void* acts, void* ts, unsigned* masks, float* out, void* gs, float* parts, int wgs, float* grads,
                           float* loss_part, int C, int nb, int N, int H, int W, int dtype, const FnResize* rz, sr_stream_t stream) {
  if (!frames || !hr || !conv_off || !acts || !out || !gs || !parts || !grads || !loss_part) return -2;
  if ((loss_kind != 1 && loss_kind != 2) || nb < 0 || N <= 0 || H <= 0 || W <= 0 || C < 1 || C > 32 || wgs < 1 || wgs > 1024) return -2;
  if (nb > 0 && (!ts || !masks)) return -2;
  if (rz && fn_resize_check(*rz) == -2) return -2;
  if (!clip_geometry_ok(nb, N, H, W, dtype, true) || (rz && fn_resize_check(*rz))) return -1;
  const long grads_n = (long)(2 * nb + 1) * (9 * C * C + C) + 75 * C + 3 + 27 * C + C;
  int rc = clip_step_check(step, grads_n, dtype);
  if (rc) return rc;
  if (step->n_idx[0] != conv_off[2 * nb + 1] + FnCfg::UP_ELEMS ||
      step->n_idx[1] != (long)(2 * nb + 1) * FnBwdCfg::CONV_ELEMS + FnBwdCfg::UP_ELEMS)
    return -2;
  hipStream_t st = (hipStream_t)stream;
  const long g_is = rz ? 3L * rz->OH * rz->OW : 48L * H * W, numel = (long)N * g_is;
  if ((rc = clip_step_prologue(step, dtype, st, rz != nullptr))) return rc;
  if (rz) {
    if ((rc = sr_fn_net_train_fwd_sized(frames, step->blob[0], conv_off, step->blob[2], acts, ts, masks, out, g_is, rz->OH, rz->OW, rz->ty,
                                        rz->ly, rz->tx, rz->lx, nb, N, H, W, dtype, SR_FN_ALL, stream)))
      return rc;
    if ((rc = sr_fn_net_bwd_loss_sized(frames, out, hr, loss_kind, 1.0f / (float)numel, loss_part, g_is, rz->OH, rz->OW, rz->ty, rz->ly,
                                       rz->tx, rz->lx, step->blob[1], acts, ts, masks, gs, parts, wgs, grads, C, nb, N, H, W, dtype,
                                       SR_FN_BWD_ALL, stream)))
      return rc;
  } else {
    if ((rc = sr_fn_net_train_fwd(frames, step->blob[0], conv_off, step->blob[2], acts, ts, masks, out, g_is, nb, N, H, W, dtype, SR_FN_ALL,
                                  stream)))
      return rc;
    if ((rc = sr_fn_net_bwd_loss(frames, out, hr, loss_kind, 1.0f / (float)numel, loss_part, g_is, step->blob[1], acts, ts, masks, gs, parts,
                                 wgs, grads, C, nb, N, H, W, dtype, SR_FN_BWD_ALL, stream)))
      return rc;
  }
  const int n_loss = (int)std::min<long>((long)N * ((H + FnBwdCfg::TH - 1) / FnBwdCfg::TH) * ((W + FnBwdCfg::TW - 1) / FnBwdCfg::TW), wgs);
  return clip_step_epilogue(step, grads, loss_part, n_loss, numel, st);
}
}  // namespace

extern "C" int sr_fn_net_train_step(const sr_clip_step_t* step, const float* frames, const float* hr, int loss_kind,
                                    const long* conv_off, void* acts, void* ts, unsigned* masks, float* out, void* gs, float* parts,
                                    int wgs, float* grads, float* loss_part, int C, int nb, int N, int H, int W, int dtype,
                                    sr_stream_t stream) {
  return fn_net_train_step_impl(step, frames, hr, loss_kind, conv_off, acts, ts, masks, out, gs, parts, wgs, grads, loss_part, C, nb, N, H,
                                W, dtype, nullptr, stream);
}

extern "C" int sr_fn_net_train_step_sized(const sr_clip_step_t* step, const float* frames, const float* hr, int loss_kind,
                                          const long* conv_off, void* acts, void* ts, unsigned* masks, float* out, int OH, int OW,
                                          const int* ty, const float* ly, const int* tx, const float* lx, void* gs, float* parts,
                                          int wgs, float* grads, float* loss_part, int C, int nb, int N, int H, int W, int dtype,
                                          sr_stream_t stream) {
  const FnResize rz{ty, ly, tx, lx, OH, OW};
  return fn_net_train_step_impl(step, frames, hr, loss_kind, conv_off, acts, ts, masks, out, gs, parts, wgs, grads, loss_part, C, nb, N, H,
                                W, dtype, &rz, stream);
}

extern "C" int sr_mf_net_train_step(const sr_clip_step_t* step, const float* frames, const float* flows, const float* flow_bound,
                                    const float* hr, int loss_kind, void* acts, void* ts, unsigned* masks, void* wf, float* out, void* gs,
                                    float* parts, int wgs, float* grads, float* loss_part, int C, int nb, int B, int N, int H, int W,
                                    int dtype, sr_stream_t stream) {
  if (!frames || !hr || !acts || !ts || !masks || !wf || !out || !gs || !parts || !grads || !loss_part) return -2;
  if ((loss_kind != 1 && loss_kind != 2) || nb < 1 || B <= 0 || N <= 0 || H <= 0 || W <= 0 || C < 1 || C > 32 || wgs < 1 || wgs > 1024)
    return -2;
  if (N > 1 && (!flows || !flow_bound)) return -2;
  if (B > 65535 || N > 65535 || !clip_geometry_ok(nb, (long)B * N, H, W, dtype, true)) return -1;
  const long grads_n = 9L * C * (2 * C + 2) + C + (long)(2 * nb - 1) * (9 * C * C + C) + 48L * 9 * C + 48 + 27 * C + C;
  int rc = clip_step_check(step, grads_n, dtype);
  if (rc) return rc;
  if (step->n_idx[0] != (long)MfCfg::FIRST_ELEMS + (long)(nb - 1) * 2 * FnCfg::CONV_ELEMS + MfCfg::DEC_ELEMS ||
      step->n_idx[1] != (long)MfBwdCfg::dec_off(nb) + MfBwdCfg::DEC_ELEMS)
    return -2;
  hipStream_t st = (hipStream_t)stream;
  const long numel = (long)B * N * 48L * H * W;
  if ((rc = clip_step_prologue(step, dtype, st))) return rc;
  if ((rc = sr_mf_net_train_fwd(frames, flows, step->blob[0], step->blob[2], acts, ts, masks, wf, out, nb, B, N, H, W, dtype, SR_MF_ALL,
                                stream)))
    return rc;
  if ((rc = sr_mf_net_bwd_loss(frames, flows, flow_bound, out, hr, loss_kind, 1.0f / (float)numel, loss_part, step->blob[1], acts, ts, masks,
                               wf, gs, parts, wgs, grads, C, nb, B, N, H, W, dtype, SR_MF_BWD_ALL, stream)))
    return rc;
  typedef MfLossCfg LC;
  const int n_loss = (int)std::min<long>((long)B * N * ((H + LC::TH - 1) / LC::TH) * ((W + LC::TW - 1) / LC::TW), wgs);
  return clip_step_epilogue(step, grads, loss_part, n_loss, numel, st);
}
