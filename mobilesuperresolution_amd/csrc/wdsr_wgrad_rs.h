// Weight gradients of conv1 / conv2 of every residual block from the saved dt images, second design (bf16, 24 units).
// Reference op: the autograd backward of Block.body[0] and body[2] (models/basic_wdsr_b.py:108-144): dW1, db1, dW2, db2.
// Products and slab layout are those of wdsr_block_wgrad_saved_kernel<ROLE 0> (wdsr_block.h); what changes is who does what:
//   * there, 15 waves = 5 e-tiles x 3 pixel splits: every wave re-reads the SAME x / dt pixel fragments its e-tile needs
//     (60 KB of LDS reads per 32-pixel tile over the workgroup, against 40 MFMAs) and a spatial tile's 9 pixel tiles never
//     divide evenly over the splits; the kernel sat at 29 % MFMA busy with half of its LDS cycles in bank conflicts;
//   * here a wave owns ALL e-tiles of its pixel tiles (10 accumulator tiles = 160 registers, 8 waves x 256 VGPRs): the four
//     pixel-major and four transposed fragments of a pixel tile are read once and serve the 40 MFMAs (28 KB with the weight
//     fragments); the layer's pixels are taken as ONE stream in the saved images' own order ([tile][288 px], contiguous), in
//     chunks of 256 pixels = one 32-pixel tile per wave, so every wave does the same work between two barriers;
//   * both images are staged by LDS-DMA (no registers, no store phase): dt as it lies, x gathered per pixel, with constant
//     16-byte chunks for the "ones" channel and the zero padding;
//   * the bias gradients cost nothing: db1 is the row of dW1 that belongs to x's ones channel, and db2 is the column of dW2
//     that belongs to one padding column of the last e-tile (E = 144 of 160), whose h is forced to 1.
#pragma once
#include "wdsr_fwd_rs.h"

// q / d for 0 <= q < n as (q * mul) >> 16: one full-rate v_mul_u32_u24 and a shift, where hipcc's constant-divisor form is a
// quarter-rate v_mul_hi plus fix-ups.  mul = 65536 / d + 1; small_div_ok() proves the range at compile time.
constexpr int small_div_mul(int d) { return 65536 / d + 1; }
constexpr bool small_div_ok(int d, int n) {
  for (int q = 0; q < n; ++q)
    if (((q * small_div_mul(d)) >> 16) != q / d) return false;
  return true;
}
template <int D> SR_DEV unsigned small_div(unsigned q) { return __umul24(q, (unsigned)small_div_mul(D)) >> 16; }
// the workgroups per layer in an SGPR for the whole kernel: hipcc re-reads gridDim.x from the dispatch packet after every
// barrier (a scalar load and its wait at the top of every chunk / tile)
SR_DEV int grid_x_once() {
  int n = __builtin_amdgcn_readfirstlane((int)gridDim.x);
  asm volatile("" : "+s"(n));
  return n;
}

template <int F, int E, int L> struct WgradA8Cfg {
  typedef BlockCfg<F, E, L> C;
  typedef BwdCfg<C> B;
  static constexpr int NWAVES = 8, NTHREADS = 64 * NWAVES, CHUNK = 32 * NWAVES;      // pixels per chunk
  static constexpr int XROW = C::KX, DROW = 32;                                        // LDS row widths (elements)
  static constexpr int X_ELEMS = CHUNK * XROW, D_ELEMS = CHUNK * DROW, BUF_ELEMS = X_ELEMS + D_ELEMS;
  static constexpr int NW1 = C::NET * C::KS1, NWL = NW1 + 2 * C::NET;
  static constexpr int LDS_BYTES = (2 * BUF_ELEMS + NWL * 512) * 2;
  static constexpr int PAD_COL = E % 32;                                               // first padding column of the last e-tile
  static_assert(C::FOLD_B1 && C::KX == 32 && C::KS1 == 2, "x rows carry the ones channel (24 units)");
  static_assert(E % 32 != 0, "needs a padding column in the last e-tile for db2");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
  static_assert(2 * BUF_ELEMS * 2 >= NWAVES * 2 * 4096, "the epilogue reuses the staging buffers for one e-tile of every wave");
  static_assert(B::NPXC % 16 == 0 && CHUNK % 16 == 0, "a 16-pixel piece lies in one tile and is whole or empty");
  static_assert(small_div_ok(C::TW, B::NPXC), "q / TW by multiplication");
};

template <int F, int E, int L>
__global__ __launch_bounds__((WgradA8Cfg<F, E, L>::NTHREADS)) void wdsr_wgrad_a8_kernel(
    const __bf16* __restrict__ act, const __bf16* __restrict__ side, const __bf16* __restrict__ wblob, float* __restrict__ partial,
    int N, int H, int W, int tiles_x, int tiles_per_img, long act_ls, long side_ls, long w_ls) {
  typedef __bf16 T;
  typedef WgradA8Cfg<F, E, L> G;
  typedef typename G::C C;
  typedef typename G::B B;
  __shared__ __attribute__((aligned(16))) char smem_raw[G::LDS_BYTES];
  T* const BUF = reinterpret_cast<T*>(smem_raw);
  T* const WL = BUF + 2 * G::BUF_ELEMS;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int layer = blockIdx.y;
  act += (size_t)layer * act_ls;
  side += (size_t)layer * side_ls;
  wblob += (size_t)layer * w_ls;
  stage_weights<T, G::NTHREADS>(WL, wblob + (size_t)C::W1_OFF * 512, G::NW1, tid);
  stage_weights<T, G::NTHREADS>(WL + G::NW1 * 512, wblob + (size_t)B::W2N_OFF * 512, 2 * C::NET, tid);
  WSrc<T, true> wsrc;
  wsrc.p = WL;

  const int total_tiles = N * tiles_per_img;
  const int total_px = total_tiles * B::NPXC;                          // (host side: N * tiles * 288 < 2^31)
  const int nchunks = (total_px + G::CHUNK - 1) / G::CHUNK;
  const char* ones = reinterpret_cast<const char*>(g_sr_const_chunks);
  const char* zeros = ones + 16;
  // One chunk = 16 pieces of x + 16 pieces of dt, two of each per wave; a piece = 16 pixels x 4 chunks of 16 bytes
  // (lane & 3 = chunk).  A chunk of 256 consecutive saved pixels touches at most two spatial tiles, and a piece lies in ONE
  // of them (288 and 256 are multiples of 16): which tile, its origin, its image and whether it exists are wave-uniform and
  // stay in SGPRs; a lane only splits its pixel number into (row, column) -- by a multiplication, TW is a constant -- and
  // forms one 64-bit address.  (Selecting the tile per lane made hipcc divide by tiles_x per lane: 50 VALU instructions per
  // x piece, 12 of them quarter-rate.)  Pixel numbers count from the layer's first pixel: N * H * W < 2^31.
  const int nwg = grid_x_once();
  const int c = lane & 3, lp = lane >> 2;
  const char* const xlane = reinterpret_cast<const char*>(act) + c * 16;
  const char* const dlane = reinterpret_cast<const char*>(side) + lp * (C::LP * 2) + c * 16;
  const char* const xfill = c == 3 ? ones : zeros;    // x rows: channels 0..23 | ones | zeros
  const bool xreal = c != 3, dreal = c < C::CPT;
  const unsigned img_px = (unsigned)H * (unsigned)W;
  auto stage = [&](int chunk, int buf) {
    T* Xb = BUF + buf * G::BUF_ELEMS;
    T* Db = Xb + G::X_ELEMS;
    const unsigned g0 = (unsigned)chunk * G::CHUNK;
    const unsigned t0 = g0 / B::NPXC, q0 = g0 - t0 * B::NPXC;
    const unsigned n0 = t0 / (unsigned)tiles_per_img, tile0 = t0 - n0 * tiles_per_img;
    const unsigned ty0 = tile0 / (unsigned)tiles_x, tx0 = tile0 - ty0 * tiles_x;
    const bool roll = tile0 + 1 == (unsigned)tiles_per_img, newrow = tx0 + 1 == (unsigned)tiles_x;
    const unsigned by0 = ty0 * C::TH, bx0 = tx0 * C::TW;
    const unsigned by1 = roll ? 0 : (newrow ? by0 + C::TH : by0), bx1 = (roll || newrow) ? 0 : bx0 + C::TW;
    const unsigned pix0 = n0 * img_px + by0 * W + bx0, pix1 = (roll ? n0 + 1 : n0) * img_px + by1 * W + bx1;
    const bool tile1 = t0 + 1 < (unsigned)total_tiles;             // (t0 itself exists: chunk < nchunks)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int piece = wave + i * G::NWAVES;
      {                                              // x: NHWC pixel of the saved order, channels 0..23 | ones | zeros
        unsigned qp = q0 + piece * 16;
        const bool wrap = qp >= (unsigned)B::NPXC;   // wave-uniform
        qp -= wrap ? B::NPXC : 0;
        const unsigned pixb = wrap ? pix1 : pix0;
        const unsigned rows = wrap ? (tile1 ? H - by1 : 0u) : H - by0, cols = wrap ? W - bx1 : W - bx0;
        const unsigned q = qp + lp;
        const unsigned oy = small_div<C::TW>(q), ox = q - __umul24(oy, C::TW);
        const bool in = xreal && oy < rows && ox < cols;
        const char* src = in ? xlane + (size_t)(pixb + oy * W + ox) * (F * 2) : xfill;
        dma_piece16(src, lds_addr(Xb) + piece * 1024);
      }
      {                                              // dt: [pixel][LP] as saved, rows padded to 32 channels
        const unsigned gp = g0 + piece * 16;         // total_px is a multiple of 16: the piece is whole or empty
        const bool in = dreal && gp < (unsigned)total_px;
        const char* src = in ? dlane + (size_t)gp * (C::LP * 2) : zeros;
        dma_piece16(src, lds_addr(Db) + piece * 1024);
      }
    }
  };

  f32x16 accA[C::NET], accB[C::NET];
#pragma unroll
  for (int et = 0; et < C::NET; ++et) { accA[et] = zero16(); accB[et] = zero16(); }

  int cur = 0;
  if ((int)blockIdx.x < nchunks) stage(blockIdx.x, 0);
  for (int ch = blockIdx.x; ch < nchunks; ch += nwg) {
    wait_vmcnt<0>();
    __syncthreads();                                 // chunk ch (and, first time, the weights) landed; the other buffer is free
    if (ch + nwg < nchunks) stage(ch + nwg, cur ^ 1);
    const T* XC = BUF + cur * G::BUF_ELEMS;
    const T* IMG = XC + G::X_ELEMS;
    const int pc = wave * 32 + r;                    // this lane's pixel row for the pixel-major fragments
    auto rowx = [=](int p) { return (wave * 32 + p) * G::XROW; };
    auto rowi = [=](int p) { return (wave * 32 + p) * G::DROW; };
    bf16x8 xa[2], da[2], xt[2], dtt[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      xa[s] = lds_chunk<T>(XC, pc * G::XROW + (2 * s + hh) * 8);
      da[s] = lds_chunk<T>(IMG, pc * G::DROW + (2 * s + hh) * 8);
      xt[s] = tr_frag<T>(XC, s, lane, rowx);
      dtt[s] = tr_frag<T>(IMG, s, lane, rowi);
    }
#pragma unroll
    for (int et = 0; et < C::NET; ++et) {
      f32x16 h2 = mma16<T>(xa[0], wsrc.get(et * 2, lane), zero16());
      h2 = mma16<T>(xa[1], wsrc.get(et * 2 + 1, lane), h2);
      f32x16 dh2 = mma16<T>(da[0], wsrc.get(G::NW1 + 2 * et, lane), zero16());
      dh2 = mma16<T>(da[1], wsrc.get(G::NW1 + 2 * et + 1, lane), dh2);
      // relu(h) and dh as bf16 fragments; the ReLU mask 1[h > 0] is applied to the PACKED dh: min(relu(h) bits, 1) is 0 / 1
      // per 16-bit half and a packed integer multiply keeps or clears dh's bit pattern -- 2 packed ops per 2 values where
      // compare + select on the fp32 accumulators cost 2 per value (this kernel is bound by VALU issue: a 32-cycle MFMA
      // hides about four VALU ops, and it had 12.6 per MFMA)
      bf16x8 hr[2] = {acc_to_frag_relu<T, 0>(h2), acc_to_frag_relu<T, 1>(h2)};
      bf16x8 dq[2] = {acc_to_frag<T, 0>(dh2), acc_to_frag<T, 1>(dh2)};
      if (et == C::NET - 1 && r == G::PAD_COL) {     // padding column e = E: relu(h) := 1, so that dW2's column there sums dt -> db2
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int j = 0; j < 8; ++j) hr[s][j] = (__bf16)1.f;
      }
      typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
#pragma unroll
      for (int s = 0; s < 2; ++s) {                  // (inline asm: hipcc expands the vector forms into compares, selects and byte permutes)
        const u32x4 hq = __builtin_bit_cast(u32x4, hr[s]);
        u32x4 dd = __builtin_bit_cast(u32x4, dq[s]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          unsigned m;
          asm volatile("v_pk_min_u16 %0, %1, %2" : "=v"(m) : "v"(hq[j]), "s"(0x00010001u));
          asm volatile("v_pk_mul_lo_u16 %0, %1, %2" : "=v"(dd[j]) : "v"(dd[j]), "v"(m));
        }
        dq[s] = __builtin_bit_cast(bf16x8, dd);
      }
      // the hazard recogniser does not see what the asm statements wrote: give the MFMAs that read dq the wait states a
      // VALU write -> MFMA read needs (without them the results were not reproducible)
      asm volatile("s_nop 4" ::: "memory");
      accA[et] = mma16<T>(xt[0], dq[0], accA[et]);
      accA[et] = mma16<T>(xt[1], dq[1], accA[et]);
      accB[et] = mma16<T>(dtt[0], hr[0], accB[et]);
      accB[et] = mma16<T>(dtt[1], hr[1], accB[et]);
    }
    cur ^= 1;
  }

  // ---- reduce the eight waves' accumulators, one e-tile at a time, through the staging buffers ----
  float* out = partial + ((size_t)layer * nwg + blockIdx.x) * B::SLAB_A;
  float* red = reinterpret_cast<float*>(smem_raw);   // [wave][2 tiles][16 regs][64 lanes]
  wait_vmcnt<0>();
#pragma unroll
  for (int et = 0; et < C::NET; ++et) {
    __syncthreads();
    slab_store_tile(red + wave * 2048, 0, accA[et], lane);
    slab_store_tile(red + wave * 2048, 1, accB[et], lane);
    __syncthreads();
    for (int i = tid; i < 2048; i += G::NTHREADS) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < G::NWAVES; ++w) v += red[w * 2048 + i];
      const int which = i >> 10, reg = (i >> 6) & 15, ln = i & 63;      // which: 0 = dW1^T tile, 1 = dW2 tile
      out[((which ? C::NET + et : et) * 16 + reg) * 64 + ln] = v;
      // db1[e] = row 24 (x's ones channel) of dW1^T: register 12 of the lanes with hh = 0, column = lane
      if (which == 0 && reg == 12 && ln < 32) out[2 * C::NET * 1024 + et * 32 + ln] = v;
      // db2[l] = column PAD_COL of the last dW2 tile: lane (PAD_COL, hh), register i -> row (i & 3) + 8 (i >> 2) + 4 hh
      if (which == 1 && et == C::NET - 1 && (ln & 31) == G::PAD_COL)
        out[2 * C::NET * 1024 + C::NET * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (ln >> 5)] = v;
    }
  }
}

// =============================================================================================
// Weight gradients of the 3x3 conv (dW3, and b3 through t's ones channel) from the saved t images, second design.
// wdsr_block_wgrad_saved_kernel<ROLE 1> gives every tap its own wave: nine waves read the SAME transposed t fragments and
// each MFMA fetches both of its operands from LDS (2 KB per MFMA; the kernel sat at 21 % MFMA busy).  Here a wave owns all
// nine taps (144 accumulator registers) of one 4x8 pixel tile of the spatial tile: t's two fragments are read once for
// 18 MFMAs, only dy's shifted fragments are per tap.  A 12x24 tile has nine pixel tiles for eight waves: the ninth is
// split by TAP (every wave holds every tap's accumulator), one tap per wave and two for wave 0, so the waves stay level.
// Both operands are staged by LDS-DMA, t as it lies, dy on its 1-pixel halo with 48-byte rows (conflict-free).
// Slab layout: that of ROLE 1 ([tap][16 regs][64 lanes]).
// =============================================================================================
template <int F, int E, int L> struct WgradB8Cfg {
  typedef BlockCfg<F, E, L> C;
  typedef BwdCfg<C> B;
  static constexpr int NWAVES = 8, NTHREADS = 64 * NWAVES;
  static constexpr int IMG_ELEMS = (B::NPXC + 1) * 32;                 // t: [core px][32 ch]
  static constexpr int PXP = 64 / C::FC;                               // dy pixels per DMA piece: 21 (63 chunks + 1 of the next pixel) / 16
  static constexpr int NPD = (C::NPXH + PXP - 1) / PXP;                // dy pieces per tile
  static constexpr int DY_ELEMS = (NPD * PXP + 1) * C::F + 32;         // dy halo tile, rows of F, + the last piece's spill
  static constexpr int NPI = B::NPXC / 16;                             // t pieces per tile (16 px x 4 chunks)
  static constexpr int BUF_ELEMS = IMG_ELEMS + DY_ELEMS;
  static constexpr int LDS_BYTES = 2 * BUF_ELEMS * 2;
  static_assert((C::FC == 3 || C::FC == 4) && C::NPT_O == 9 && B::NPXC % 16 == 0, "24 or 32 units, 12x24 tiles");
  static_assert(LDS_BYTES >= NWAVES * 2 * 4096, "the epilogue reduces two taps of every wave at a time in the staging buffers");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
  static_assert(small_div_ok(C::HW, (NPD + 1) * PXP), "halo pixel / HW by multiplication");
};

template <int F, int E, int L>
__global__ __launch_bounds__((WgradB8Cfg<F, E, L>::NTHREADS)) void wdsr_wgrad_b8_kernel(
    const __bf16* __restrict__ dyact, const __bf16* __restrict__ side, float* __restrict__ partial, int N, int H, int W,
    int tiles_x, int tiles_per_img, long act_ls, long side_ls) {
  typedef __bf16 T;
  typedef WgradB8Cfg<F, E, L> G;
  typedef typename G::C C;
  typedef typename G::B B;
  __shared__ __attribute__((aligned(16))) char smem_raw[G::LDS_BYTES];
  T* const BUF = reinterpret_cast<T*>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int layer = blockIdx.y;
  dyact += (size_t)layer * act_ls;
  side += (size_t)layer * side_ls;
  const int total = N * tiles_per_img;
  const char* zeros = reinterpret_cast<const char*>(g_sr_const_chunks) + 16;

  // The pieces of a tile are dealt to the waves round-robin; the loop over them is unrolled, so which kind a piece is falls out at
  // compile time or is a wave-uniform branch.  What a lane contributes (its pixel and chunk inside a piece) is fixed for the
  // kernel; per piece it splits one halo pixel number into (row, column) by a multiplication -- HW is a constant -- and forms
  // one address.  (Rolled up, every piece took a quarter-rate v_mul_hi, two 64-bit multiply-adds and three branches.)
  const int nwg = grid_x_once();
  const int lq = lane / C::FC, lc = lane - lq * C::FC;               // dy pieces: PXP pixels x FC chunks
  const char* const tlane = reinterpret_cast<const char*>(side) + (lane >> 2) * (C::LP * 2) + (lane & 3) * 16;
  const char* const dylane = reinterpret_cast<const char*>(dyact) + lc * 16;
  const bool treal = (lane & 3) < C::CPT;                            // t pieces: 16 pixels x (CPT chunks + zero chunks)
  auto stage = [&](int t, int buf) {
    T* IMGb = BUF + buf * G::BUF_ELEMS;
    T* DYb = IMGb + G::IMG_ELEMS;
    const unsigned n = (unsigned)t / (unsigned)tiles_per_img, tile = t - n * tiles_per_img;
    const unsigned ty = tile / (unsigned)tiles_x, tx = tile - ty * tiles_x;
    const unsigned hy0 = ty * C::TH - 1, hx0 = tx * C::TW - 1;       // the halo's origin; -1 wraps and fails the bounds below
    const char* tsrc = tlane + (size_t)t * (B::NPXC * C::LP * 2);
    const char* dimg = dylane + (size_t)n * H * W * (F * 2);
#pragma unroll
    for (int i = 0; i < (G::NPI + G::NPD + G::NWAVES - 1) / G::NWAVES; ++i) {
      const int p = wave + i * G::NWAVES;
      if (p < G::NPI) {                              // t: 16 pixels x (3 chunks + a zero chunk) per piece, rows of 32 channels
        const char* src = treal ? tsrc + p * (16 * C::LP * 2) : zeros;
        dma_piece16(src, lds_addr(IMGb) + p * 1024);
      } else if (p < G::NPI + G::NPD) {              // dy on the 1-pixel halo: 21 pixels x 3 chunks (+ 1 chunk the next piece rewrites), or 16 x 4
        const int q = p - G::NPI;
        const unsigned hp = q * G::PXP + lq;
        const unsigned hy = small_div<C::HW>(hp), hx = hp - __umul24(hy, C::HW);
        const unsigned Y = hy0 + hy, X = hx0 + hx;
        const bool in = hp < (unsigned)C::NPXH && Y < (unsigned)H && X < (unsigned)W;
        const char* src = in ? dimg + (size_t)(Y * W + X) * (F * 2) : zeros;
        dma_piece16(src, lds_addr(DYb) + q * (G::PXP * C::F * 2));
      }
    }
  };

  f32x16 acc[9];
#pragma unroll
  for (int u = 0; u < 9; ++u) acc[u] = zero16();

  // The transposed fragments of a 4x8 pixel tile (tr_frag's element order: k-step s takes pixel rows 2s and 2s + 1 of the
  // tile, a lane supplies the address of column 4 hh + q).  The address of a read is (buffer + the tile's corner + the lane's
  // part) + a compile-time offset for the row and the tap: the first part is made once per tile and hidden from the optimiser,
  // so that the 36 dy reads of a tile carry their offsets as immediates (hipcc kept 22 per-lane registers, one per row and tap,
  // and spent a v_add on every read).
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  const int lane_px = 4 * (lane >> 5) + ((lane >> 2) & 3), lane_ch = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  auto frag_base = [](const T* p) {
    unsigned a = lds_addr(p);
    asm volatile("" : "+v"(a));
    return (const lds_bf16x4*)(size_t)a;
  };
  auto frag = [](const lds_bf16x4* base, int lo_elems, int hi_elems) {
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(const_cast<lds_bf16x4*>(base) + lo_elems / 4);
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(const_cast<lds_bf16x4*>(base) + hi_elems / 4);
    bf16x8 f;
    f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3];
    f[4] = hi[0]; f[5] = hi[1]; f[6] = hi[2]; f[7] = hi[3];
    return f;
  };
  auto t_frag = [&](const lds_bf16x4* base, int s) { return frag(base, 2 * s * C::TW * 32, (2 * s + 1) * C::TW * 32); };
  auto dy_frag = [&](const lds_bf16x4* base, int s, int uy, int ux) {
    return frag(base, ((2 * s + uy) * C::HW + ux) * C::F, ((2 * s + 1 + uy) * C::HW + ux) * C::F);
  };

  int cur = 0;
  if ((int)blockIdx.x < total) stage(blockIdx.x, 0);
  for (int t = blockIdx.x; t < total; t += nwg) {
    wait_vmcnt<0>();
    __syncthreads();
    if (t + nwg < total) stage(t + nwg, cur ^ 1);
    const T* IMG = BUF + cur * G::BUF_ELEMS;
    const T* DYs = IMG + G::IMG_ELEMS;
    {                                                // this wave's own pixel tile: all nine taps
      const int ot = wave;
      const int toy = (ot / (C::TW / 8)) * 4, tox = (ot % (C::TW / 8)) * 8;
      const lds_bf16x4* tb = frag_base(IMG + (toy * C::TW + tox + lane_px) * 32 + lane_ch);
      const lds_bf16x4* db = frag_base(DYs + (toy * C::HW + tox + lane_px) * C::F + lane_ch);
      const bf16x8 a0 = t_frag(tb, 0), a1 = t_frag(tb, 1);
#pragma unroll
      for (int u = 0; u < 9; ++u) {
        const int uy = u / 3, ux = u - uy * 3;
        acc[u] = mma16<T>(a0, dy_frag(db, 0, uy, ux), acc[u]);
        acc[u] = mma16<T>(a1, dy_frag(db, 1, uy, ux), acc[u]);
      }
    }
    {                                                // the ninth pixel tile, split by tap: tap = wave (and tap 8 for wave 0)
      constexpr int ot = 8;
      constexpr int toy = (ot / (C::TW / 8)) * 4, tox = (ot % (C::TW / 8)) * 8;
      const lds_bf16x4* tb = frag_base(IMG + (toy * C::TW + tox + lane_px) * 32 + lane_ch);
      const lds_bf16x4* db = frag_base(DYs + (toy * C::HW + tox + lane_px) * C::F + lane_ch);
      const bf16x8 a0 = t_frag(tb, 0), a1 = t_frag(tb, 1);
#pragma unroll
      for (int u = 0; u < 9; ++u) {
        if (u == wave || (u == 8 && wave == 0)) {    // wave-uniform
          const int uy = u / 3, ux = u - uy * 3;
          acc[u] = mma16<T>(a0, dy_frag(db, 0, uy, ux), acc[u]);
          acc[u] = mma16<T>(a1, dy_frag(db, 1, uy, ux), acc[u]);
        }
      }
    }
    cur ^= 1;
  }

  // ---- reduce the eight waves' accumulators, two taps at a time, through the staging buffers ----
  float* out = partial + ((size_t)layer * nwg + blockIdx.x) * B::SLAB_B;
  float* red = reinterpret_cast<float*>(smem_raw);   // [wave][2 taps][16 regs][64 lanes]
  wait_vmcnt<0>();
#pragma unroll
  for (int u0 = 0; u0 < 9; u0 += 2) {
    __syncthreads();
    slab_store_tile(red + wave * 2048, 0, acc[u0], lane);
    if (u0 + 1 < 9) slab_store_tile(red + wave * 2048, 1, acc[u0 + 1 < 9 ? u0 + 1 : 8], lane);
    __syncthreads();
    const int nval = u0 + 1 < 9 ? 2048 : 1024;
    for (int i = tid; i < nval; i += G::NTHREADS) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < G::NWAVES; ++w) v += red[w * 2048 + i];
      out[u0 * 1024 + i] = v;
    }
  }
}
