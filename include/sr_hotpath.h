/* sr_hotpath.h -- C ABI of libsr_hotpath.so: the MI355X (gfx950) kernels behind the
 * WDSR-B / BasicVSR super-resolution hot path of zhuzhui-2000/mobilesuperresolution.
 *
 * The reference has no FFI of its own: its boundary is the nn.Module surface
 * (models/__init__.py:31-32 get_model, models/basic_wdsr_b.py:85-93 BASIC_MODEL.forward).  This
 * header is the seam *beneath* that surface: the Python mirror in mobilesuperresolution_amd/models
 * binds these entry points with ctypes (see INTEGRATION.md for the binding a maintainer would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer borrowed from the caller (PyTorch allocator); nothing is
 *     allocated, freed or synchronised inside; all work is enqueued on `stream` (a hipStream_t).
 *   - activations are NHWC ("pixel-major, channels innermost"); dtype: 0 = float32 (exact-fp32 MFMA,
 *     parity mode), 1 = bfloat16 storage with fp32 accumulation (throughput mode).
 *   - weights arrive as "packed fragment blobs" built on the host by
 *     mobilesuperresolution_amd/packing.py from the effective (weight-normalised) tensors.
 *   - return value: 0 on success, a hipError_t value on a launch error, -1 unsupported geometry,
 *     -2 bad argument.  Entry points are re-entrant and hold no global mutable state (autograd calls
 *     the backward ones from its own thread).
 */
#ifndef SR_HOTPATH_H
#define SR_HOTPATH_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sr_stream_t; /* hipStream_t */

#define SR_DTYPE_F32 0
#define SR_DTYPE_BF16 1

/* ABI version of this header: 25(bumped on any signature change). */
int sr_abi_version(void);

/* Fused residual block forward.  Replaces Block.forward, models/basic_wdsr_b.py:142-144 (body of
 * :108-138): y = conv3x3(conv1x1(relu(conv1x1(x)))) + x on an N x H x W x F NHWC tensor.
 * Supported (F, E, L): (24,144,20), (32,192,26).  wblob / cinit: packing.block_fwd_tables(). */
int sr_wdsr_block_fwd(const void* x, void* y, const void* wblob, const float* cinit,
                      int N, int H, int W, int F, int dtype, sr_stream_t stream);

/* Two consecutive residual blocks in one launch (bf16, F = 24 or 32; -1 otherwise): x -> ya (block A's
 * output, kept because backward needs every block input; NULL = do not store) -> yb.  Equal to two sr_wdsr_block_fwd
 * calls up to the fp32 summation order of the 3x3 conv (dense-K form: the residual enters the sum first); exists because a
 * single block launch at batch 32 is bound by its fixed costs.  (= sr_wdsr_fwd_rs with nblk = 2.) */
int sr_wdsr_block2_fwd(const void* x, void* ya, void* yb, const void* wblob_a, const void* wblob_b,
                       const float* cinit_a, const float* cinit_b, void* tsave_a, void* tsave_b, int N, int H, int W,
                       int F, int dtype, sr_stream_t stream);
/* tsave_a / tsave_b (NULL = off): keep each block's t = conv1x1(relu(conv1x1(x))) (the 3x3 conv's input,
 * basic_wdsr_b.py:131-137) for the core pixels, tile-local [N][tiles][288][24] bf16, for
 * sr_wdsr_block_wgrad_saved. */

/* Backward-data of two consecutive blocks in one launch (bf16, F = 24 or 32; -1 otherwise): block A feeds
 * block B.  xa / xb = the blocks' inputs, dyb = gradient at B's output; writes dxb (= gradient at A's
 * output, which the weight-gradient kernels read) and dxa.  F = 32: bit-identical to two sr_wdsr_block_bwd_data calls
 * (csrc/wdsr_bwd_pair_lds.h); F = 24: equal to them up to fp32 summation order (csrc/wdsr_bwd_rs.h: the skip term enters the sum
 * first). */
int sr_wdsr_block2_bwd_data(const void* xa, const void* xb, const void* dyb, void* dxb, void* dxa,
                            const void* wblob_a, const void* wblob_b, const float* cinit_a, const float* cinit_b,
                            void* dtsave_a, void* dtsave_b, int N, int H, int W, int F, int dtype, sr_stream_t stream);
/* dtsave_a / dtsave_b (NULL = off): keep each block's dt = conv3x3^T(dy), same layout as tsave.
 *
 * Weight gradients of `layers` blocks from the saved t / dt images instead of recomputing them (bf16 only;
 * -1 otherwise).  Same slabs as sr_wdsr_block_wgrad.  side_ls = elements between two blocks' saved images
 * ([N][tiles][288][LP], LP = 24 for 24 units, 32 for 32 units). */
int sr_wdsr_block_wgrad_saved(const void* x, const void* dy, const void* tsave, const void* dtsave,
                              const void* wblob, const float* cinit, float* partial_a, float* partial_b, int layers,
                              int wgs, int N, int H, int W, int F, int dtype, long x_ls, long dy_ls, long side_ls,
                              long w_ls, long c_ls, sr_stream_t stream);

/* Forward of nblk = 1 or 2 consecutive residual blocks, role-specialised kernels of csrc/wdsr_fwd_rs.h /
 * wdsr_fwd_stream.h (bf16; -1 otherwise).  F = 24: every wave keeps the weights of its current phase in registers, x / weights
 * are staged by LDS-DMA; from 256 whole images of width 48 on, the streaming kernel.  F = 32: sixteen waves, weights read from
 * LDS at use.  The 3x3 conv runs in its dense-K form.  Same arguments as sr_wdsr_block_fwd (nblk = 1: x -> yb, the *_b / ya
 * arguments unused) and sr_wdsr_block2_fwd (nblk = 2); results equal to theirs up to fp32 summation order, and bit-identical
 * across this entry point's kernels (one- and two-block launches, tile, persistent and streaming forms). */
int sr_wdsr_fwd_rs(const void* x, void* ya, void* yb, const void* wblob_a, const void* wblob_b, const float* cinit_a,
                   const float* cinit_b, void* tsave_a, void* tsave_b, int nblk, int N, int H, int W, int F, int dtype,
                   sr_stream_t stream);
/* measurement aid: `reps` back-to-back launches ping-ponging x <-> yb; tsave_a / tsave_b as in sr_wdsr_fwd_rs (NULL: the
 * inference variant; both given: the variant a training step launches, which also keeps the t images) */
int sr_wdsr_fwd_rs_repeat(void* x, void* ya, void* yb, const void* wblob_a, const void* wblob_b, const float* cinit_a,
                          const float* cinit_b, void* tsave_a, void* tsave_b, int nblk, int N, int H, int W, int F, int dtype,
                          int reps, sr_stream_t stream);

/* Measurement aid for bench.py's roofline leg: `reps` back-to-back launches of the same forward kernel,
 * ping-ponging x <-> y, so that HIP events around the call measure the kernel and not the host. */
int sr_wdsr_block_fwd_repeat(void* x, void* y, const void* wblob, const float* cinit,
                             int N, int H, int W, int F, int dtype, int reps, sr_stream_t stream);
/* Same for the two-block kernel: launch i reads x (even i) or yb (odd i), writes ya and the other one. */
int sr_wdsr_block2_fwd_repeat(void* x, void* ya, void* yb, const void* wblob_a, const void* wblob_b,
                              const float* cinit_a, const float* cinit_b, int N, int H, int W, int F, int dtype,
                              int reps, sr_stream_t stream);


/* Fused residual block backward w.r.t. its input.  Replaces autograd's backward of Block.forward
 * (models/basic_wdsr_b.py:142-144): dx = dy + W1^T[1(h>0) * W2^T conv3x3^T(dy)], h recomputed from x.
 * wblob / cinit: packing.block_tables() (forward sections first). */
int sr_wdsr_block_bwd_data(const void* x, const void* dy, void* dx, const void* wblob, const float* cinit,
                           int N, int H, int W, int F, int dtype, sr_stream_t stream);

/* Weight/bias gradients of `layers` residual blocks in one call.  Layer i reads x + i*x_ls,
 * dy + i*dy_ls, wblob + i*w_ls, cinit + i*c_ls (strides in elements).  Every workgroup writes one
 * partial slab: partial_a[layers][wgs_per_layer][slab_a] (dW1, dW2, db1, db2) and
 * partial_b[layers][wgs_per_layer][slab_b] (dW3, db3) in accumulator layout; the caller sums over
 * the workgroup axis and gathers with packing.block_grad_tables().  sr_wdsr_block_slab_sizes returns
 * the slab lengths (floats). */
int sr_wdsr_block_wgrad(const void* x, const void* dy, const void* wblob, const float* cinit,
                        float* partial_a, float* partial_b, int layers, int wgs_per_layer,
                        int N, int H, int W, int F, int dtype,
                        long x_ls, long dy_ls, long w_ls, long c_ls, sr_stream_t stream);
int sr_wdsr_block_slab_sizes(int F, int* slab_a, int* slab_b);

/* Head conv forward.  Replaces `x - image_mean` + self.head(x), models/basic_wdsr_b.py:86-87:
 * x NCHW fp32 [N,3,H,W] in [0,1] -> y NHWC [N,H,W,F].  wblob: packing.ends_tables()["head"]. */
int sr_head_fwd(const float* x_nchw, void* y, const void* wblob, float mean, int N, int H, int W, int F,
                int dtype, sr_stream_t stream);
/* Fused tail: self.tail(y) + self.skip(x - mean) -> PixelShuffle(R) -> + mean, models/basic_wdsr_b.py:90-92.
 * feat NHWC [N,H,W,F], x NCHW fp32, out NCHW fp32 [N,3,R*H,R*W].  R in {2,3,4}.
 * wblob: packing.ends_tables()["tail"] (forward section, then the backward-data section). */
int sr_tail_fwd(const void* feat, const float* x_nchw, float* out, const void* wblob, float mean,
                int N, int H, int W, int F, int R, int dtype, sr_stream_t stream);
/* d(loss)/d(feat) of the tail from d(loss)/d(out) (NCHW fp32, HR). */
int sr_tail_bwd_data(const float* dout, void* dfeat, const void* wblob, int N, int H, int W, int F, int R,
                     int dtype, sr_stream_t stream);
/* Weight/bias gradients of tail + skip: partial[wgs][14*NT*1024] floats in accumulator layout
 * (packing.ends_grad_tables()["tail"]); NT = ceil(3 R^2 / 32). */
int sr_tail_wgrad(const float* dout, const void* feat, const float* x_nchw, float mean, float* partial,
                  int wgs, int N, int H, int W, int F, int R, int dtype, sr_stream_t stream);
/* sr_tail_bwd_data + sr_tail_wgrad in one launch (bf16 only; -1 otherwise): reads the HR gradient once.
 * Same outputs, bit for bit, as the two calls with the same `wgs`. */
int sr_tail_bwd(const float* dout, const void* feat, const float* x, float mean, const void* wblob, void* dfeat,
                float* partial, int wgs, int N, int H, int W, int F, int R, int dtype, sr_stream_t stream);
/* Weight/bias gradient of the head conv from dy0 = d(loss)/d(head output), NHWC: partial[wgs][3*1024]. */
int sr_head_wgrad(const void* dy0, const float* x_nchw, float mean, float* partial, int wgs,
                  int N, int H, int W, int F, int dtype, sr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * BasicVSR propagation trunk: 3x3 convolutions of ConvResidualBlocks / ResidualBlockNoBN,
 * models/basicvsr_arch.py:108-147.  NHWC activations, CI in {24, 32} input channels (the 27-channel
 * concat of frame + state is stored zero-padded to 32), 24 output channels.  act: 0 none, 1 ReLU,
 * 2 LeakyReLU(0.1).  wblob: packing.c3_tables() (forward fragments, then backward-data fragments).
 * ------------------------------------------------------------------------------------------------ */
/* y = act(conv3x3(x) + b) (+ res when res != NULL; only with act == 0). */
int sr_c3_fwd(const void* x, const void* res, void* y, const void* wblob, int N, int H, int W, int CI, int act,
              int dtype, sr_stream_t stream);
/* dx = conv3x3^T(dA * act'(A)) (+ add when add != NULL; only with act == 1).  A = saved post-activation
 * output (ignored for act == 0). */
int sr_c3_bwd_data(const void* dA, const void* A, const void* add, void* dx, const void* wblob, int N, int H,
                   int W, int CI, int act, int dtype, sr_stream_t stream);
/* weight/bias gradient slabs partial[wgs][9*1024] (accumulator layout, packing.c3_grad_table()). */
int sr_c3_wgrad(const void* x, const void* dA, const void* A, float* partial, int wgs, int N, int H, int W,
                int CI, int act, int dtype, sr_stream_t stream);

/* The first conv's input gathered on the fly: what the reference builds per frame and direction as
 * `flow_warp(feat_prop, flow.permute(0,2,3,1))` then `torch.cat([x_i, feat_prop], dim=1)` (models/basicvsr_arch.py:74-76,
 * 85-87; mvvsr_arch.py:79-81,90-92).  frame [N][3][H][W] fp32 (batch stride frame_bs elements); state [N][H][W][24] in the
 * hot dtype = the previous call's a_nb (NULL: zero state, the first frame of a direction); flow [N][2][H][W] fp32, x then
 * y displacement, batch stride flow_bs (NULL: no warp).  Backward only: flow_bound = device scalar >= max |flow| (read by
 * the kernel, no host sync; it sizes the gather window of the atomics-free d state); dstate [N][H][W][24] hot dtype (NULL:
 * not wanted); dflow [N][2][H][W] fp32 with batch stride dflow_bs (NULL: not wanted). */
typedef struct sr_c3_warp {
  const float* frame; long frame_bs;
  const void* state;
  const float* flow; long flow_bs;
  const float* flow_bound;
  void* dstate;
  float* dflow; long dflow_bs;
  void* x0_save;   /* optional [N][H][W][32] hot dtype: forward writes the gathered input there, backward reads it for the
                      first conv's weight gradient instead of gathering again */
} sr_c3_warp_t;

/* Slabs -> gradient of the trunk's flat parameter inside sr_c3_trunk_bwd (NULL: the caller reduces `parts` itself):
 * gflat[off_k + i] = sum_w parts[k][w][sidx[i]], conv 0 through sidx0 (n0 elements), convs 1..2nb through sidx1 (n1
 * elements each, consecutive in gflat from element n0 on). */
typedef struct sr_c3_unpack {
  const int* sidx0; const int* dst0; int n0;
  const int* sidx1; const int* dst1; int n1;
  float* gflat;
} sr_c3_unpack_t;

/* The whole propagation trunk, ConvResidualBlocks.forward (models/basicvsr_arch.py:108-147), from one call.
 * Input: EITHER x0 [N,H,W,ci0] (ci0 = 32: the 27-channel concat zero-padded, or 24) OR warp (frame, state, flow; ci0 = 32)
 * -- exactly one of the two is non-NULL.  acts [(nb+1)][N,H,W,24] receives a_0..a_nb (a_nb = output), mids [nb][N,H,W,24]
 * the post-ReLU conv1 outputs; blob = every conv's packed weights in one buffer, conv k (0 = first conv, 1+2i / 2+2i =
 * conv1 / conv2 of block i) at ELEMENT offset blob_off[k] (host array).
 * TWO TRUNKS IN ONE CALL (n_dir > 0; the two time directions of a BasicVSR frame step, basicvsr_arch.py:67-88, are independent):
 * images [0, n_dir) of the batch run through the trunk whose packed weights sit at `blob`, images [n_dir, N) through the one
 * `blob_dir_stride` ELEMENTS behind it (same layout, same blob_off); n_dir = 0: one trunk. */
int sr_c3_trunk_fwd(const void* x0, const sr_c3_warp_t* warp, void* acts, void* mids, const void* blob,
                    const long* blob_off, int nb, int N, int H, int W, int ci0, int dtype, int n_dir, long blob_dir_stride,
                    sr_stream_t stream);
/* Its backward.  ga [(nb+1)][N,H,W,24]: the caller writes d(loss)/d(a_nb) into slot nb, the call fills the other
 * slots; gt [nb][...] scratch (gradients at the post-ReLU points); parts [(1+2nb)][wgs][9*1024] fp32 weight-gradient
 * slabs per conv (layout packing.c3_tables "grad"); dx0 (may be NULL unless warp->dstate / dflow is asked for) =
 * gradient w.r.t. the first conv's 32-channel input.
 * n_dir > 0 (two trunks, as in sr_c3_trunk_fwd): wgs must be even -- the first wgs / 2 slabs of every conv sum over the first trunk's
 * images, the others over the second's -- and unpack->gflat receives the two trunks' gradients one behind the other. */
int sr_c3_trunk_bwd(const void* x0, const sr_c3_warp_t* warp, const void* acts, const void* mids, void* ga, void* gt,
                    const void* blob, const long* blob_off, float* parts, void* dx0, const sr_c3_unpack_t* unpack, int nb,
                    int wgs, int N, int H, int W, int ci0, int dtype, int n_dir, long blob_dir_stride, sr_stream_t stream);

/* The 64-feature propagation trunk, INFERENCE only (ConvResidualBlocks with 24 < F <= 64, embedded in 64 channels; csrc/conv64.h).
 * Input: EITHER x0 [N,H,W,ci0] in the hot dtype (ci0 = 80: state 0..63 | frame 64..66 | zeros, the (F + 3)-channel concat as the
 * kernels lay it out; or ci0 = 64) OR warp (frame, state [N,H,W,64], flow; ci0 = 80; dstate, dflow and x0_save must be NULL) --
 * exactly one of the two.  Caller-owned scratch: ping, pong [N,H,W,64] (may be NULL when nb = 0); out [N,H,W,64] receives the
 * trunk's output (the next call's state; it must not be the state read by this call).  blob / blob_off as sr_c3_trunk_fwd, conv k
 * packed by packing.c64_tables; n_dir / blob_dir_stride as sr_c3_trunk_fwd.  No saved activations, no backward. */
int sr_c64_trunk_fwd(const void* x0, const sr_c3_warp_t* warp, void* ping, void* pong, void* out, const void* blob,
                     const long* blob_off, int nb, int N, int H, int W, int ci0, int dtype, int n_dir, long blob_dir_stride,
                     sr_stream_t stream);

/* The 64-feature propagation trunk, TRAINING route (opt-in: ConvResidualBlocks.hot_training; csrc/conv64.h, csrc/conv64_bwd.h).
 * The arguments mirror sr_c3_trunk_fwd at 64 channels: x0 [N,H,W,ci0] (ci0 = 80 or 64, laid out as for sr_c64_trunk_fwd) OR warp
 * (ci0 = 80; warp->x0_save, optional, [N,H,W,80] receives the gathered input); acts [(nb+1)][N,H,W,64] receives a_0..a_nb, mids
 * [nb][N,H,W,64] the post-ReLU conv1 outputs.  Both dtypes run conv1 and conv2 of a block as two launches; the result equals
 * sr_c64_trunk_fwd's bit for bit. */
int sr_c64_trunk_train_fwd(const void* x0, const sr_c3_warp_t* warp, void* acts, void* mids, const void* blob,
                           const long* blob_off, int nb, int N, int H, int W, int ci0, int dtype, int n_dir,
                           long blob_dir_stride, sr_stream_t stream);
/* Its backward; the arguments mirror sr_c3_trunk_bwd.  ga [(nb+1)][N,H,W,64]: the caller writes d(loss)/d(a_nb) into slot nb; gt
 * [nb][...] scratch.  bwd_blob: packing.c64_trunk_bwd_tables -- per conv the flipped, transposed weights in the forward fragment
 * layout with zero bias; bwd_blob_off has 2 + 2 nb entries: conv k at [k] (conv 0: its state / plain-input half), and at [1 + 2 nb]
 * the frame half of conv 0 (ci0 = 80), negative when the frame gradient is not wanted.  dx0 (NULL: no input gradient): [N,H,W,64]
 * gradient of the state (warp: of the WARPED state) or of the 64-channel input, followed, when the frame half runs, by a second
 * [N,H,W,64] image whose channels 0..2 are the frame gradient.  warp->dstate [N,H,W,64] (needs dx0, warp->state, and flow_bound
 * with a flow) receives the gradient of the state through the gather-form warp backward; warp->dflow [N][2][H][W] fp32, batch
 * stride warp->dflow_bs (needs dx0, warp->state and warp->flow; H W <= 2^30) receives the gradient of the flow, written, not
 * accumulated (sr_c64_warp_dflow below, launched after conv 0's backward-data).  parts (NULL: no weight gradient): fp32 slabs, conv 0 [wgs][54 * 1024] (ci0 = 80) or [wgs][38 * 1024],
 * then convs 1..2nb [wgs][38 * 1024] each; with warp the first conv's weight gradient reads warp->x0_save.  unpack / n_dir / wgs as
 * sr_c3_trunk_bwd (tables: packing.c64_trunk_bwd_tables; gflat holds the REAL parameter entries only). */
int sr_c64_trunk_bwd(const void* x0, const sr_c3_warp_t* warp, const void* acts, const void* mids, void* ga, void* gt,
                     const void* bwd_blob, const long* bwd_blob_off, float* parts, void* dx0, const sr_c3_unpack_t* unpack, int nb,
                     int wgs, int N, int H, int W, int ci0, int dtype, int n_dir, long bwd_dir_stride, sr_stream_t stream);

/* The flow gradient of the gathered first conv alone (c64_warp_dflow_kernel, csrc/conv64_bwd.h): for every output pixel o
 * dflow[o] = sum_c g[o][c] * d(bilinear(state, pos(o)))/d(pos), with pos and the taps computed as the forward gather computes them.
 * g [N,H,W,64]: the state half of dx0; state [N,H,W,64]: the image the forward warped (both in the hot dtype, channels >= F zero);
 * flow [N][2][H][W] fp32, batch stride flow_bs; dflow fp32 [N][2][H][W], batch stride dflow_bs, written.  A corner outside the
 * image contributes 0; the x component is 0 when W == 1, the y component when H == 1.  -2: a NULL pointer, a dtype other than
 * bf16 / fp32, N > 65535 or H W > 2^30.  Added without a change of sr_abi_version(): an addition, and a caller that left
 * warp->dflow NULL in sr_c64_trunk_bwd (the only value it accepted before) sees no difference. */
int sr_c64_warp_dflow(const void* g, const void* state, const float* flow, long flow_bs, float* dflow, long dflow_bs, int N,
                      int H, int W, int dtype, sr_stream_t stream);

/* The reconstruction of BasicVSR_origin, INFERENCE only (csrc/vsr_recon.h): fusion (1x1, 2F -> F) -> upconv1 + PixelShuffle(2) ->
 * upconv2 + PixelShuffle(2) -> conv_hr (LeakyReLU(0.1) after each) -> conv_last + bilinear x4 of the input frame.
 * feat_b, feat_f [N,H,W,cw]: the two trunks' NHWC state images in the hot dtype, cw = 64 (sr_c64_trunk_fwd's out) or 24
 * (sr_c3_trunk_fwd's last activation); channels >= F must be zero.  frame: fp32 [3,H,W] per image, images frame_bs floats apart.
 * blob / blob_off[5]: packing.c64_recon_tables (fusion, upconv1, upconv2, conv_hr, conv_last).  Caller-owned scratch in the hot
 * dtype: fused [N,H,W,64], up1 [N,2H,2W,64], up2 and hr [N,4H,4W,64], all distinct.  out: fp32 [3,4H,4W] per image, images
 * out_bs floats apart (a slice of a larger tensor).  stages: bit k runs layer k of the five on the scratch images as they are
 * (31 = the whole reconstruction; single bits serve tests and timing). */
int sr_c64_recon_fwd(const void* feat_b, const void* feat_f, int cw, const float* frame, long frame_bs, const void* blob,
                     const long* blob_off, void* fused, void* up1, void* up2, void* hr, float* out, long out_bs, int N, int H,
                     int W, int dtype, int stages, sr_stream_t stream);
/* Backward of sr_c64_recon_fwd at cw = 64 (24 < F <= 64; csrc/vsr_recon_bwd.h), one frame of every clip per call.  feat_b / feat_f
 * and fused, up1, up2, hr: what the forward read and left (kept per frame).  g: d loss / d out, fp32 [3,4H,4W] per image, images
 * g_bs floats apart.  bwd_blob = packing.c64_recon_bwd_tables(F) in the hot dtype, blob_off its six section offsets.  d_hr, d_up2
 * [N,4H,4W,64], d_up1 [N,2H,2W,64], d_fused [N,H,W,64]: caller-owned gradient images in the hot dtype (d_hr = conv_last^T(g) *
 * lrelu'(hr); the other three unmasked: the next stage's staging applies lrelu').  dfeat_b / dfeat_f [N,H,W,64]: the two state
 * gradients, all 64 channels written (channels >= F exactly zero).  parts: wgs * sr_c64_recon_bwd_slab() floats of weight-gradient
 * slabs, plain stores.  stages: bit k runs the backward of layer k (the forward's bits; 31 = all, in the order 16, 8, 4, 2, 1).
 * sr_c64_recon_reduce sums the slabs in workgroup order into grads -- the ten parameters' gradients in nn.Conv2d layout, flattened
 * in state_dict order; table = packing.c64_recon_bwd_tables(F)["reduce"] (int32, n entries); accumulate != 0 adds to grads (the
 * frames of a clip, in call order); N, H, W as in the backward call.  No allocation, no synchronisation, no float atomics.
 * -2 (a null pointer a stage needs, wgs outside 1..1024, sizes out of range) leaves every buffer untouched.  Added without a change
 * of sr_abi_version(). */
int sr_c64_recon_bwd(const void* feat_b, const void* feat_f, const void* fused, const void* up1, const void* up2, const void* hr,
                     const float* g, long g_bs, const void* bwd_blob, const long* blob_off, void* d_hr, void* d_up2, void* d_up1,
                     void* d_fused, void* dfeat_b, void* dfeat_f, float* parts, int wgs, int N, int H, int W, int dtype, int stages,
                     sr_stream_t stream);
int sr_c64_recon_bwd_slab(void);
int sr_c64_recon_reduce(const float* parts, int wgs, const int* table, int n, float* grads, int accumulate, int N, int H, int W,
                        sr_stream_t stream);

/* The reconstruction of MotionVectorVSR, forward and backward (csrc/mv_recon.h): 1x1 fusion (2F -> 2F) + LeakyReLU(0.1) ->
 * ConvTranspose2d(2F, 3, 5, stride 4) -> bilinear resize (4H+1, 4W+1) -> (4H, 4W) -> + bilinear x4 of the input frame, the whole
 * clip per call.  feat_b / feat_f: HOST arrays of NF device pointers, frame i's backward / forward state image [B,H,W,cw] in the
 * hot dtype (cw = 24 or 64; channels >= F zero).  x: fp32, frame i of clip n at x + n x_bs + i x_fs, a dense [3,H,W] block.
 * blob: packing.mv_recon_tables.  out: fp32, frame i of clip n at out + n out_bs + i out_fs, a dense [3,4H,4W] block.
 * u_save: NULL, or [NF,B,H,W,2cw] in the hot dtype, receives the fused activation (what the backward needs). */
int sr_mv_recon_fwd(const void* const* feat_b, const void* const* feat_f, int cw, const float* x, long x_bs, long x_fs,
                    const void* blob, float* out, long out_bs, long out_fs, void* u_save, int NF, int B, int H, int W, int dtype,
                    sr_stream_t stream);
/* Backward of sr_mv_recon_fwd, cw = 24 only.  g: the gradient at `out`, laid out like it (g_bs, g_fs).  dfeat_b / dfeat_f: HOST
 * arrays of NF device pointers to [B,H,W,24] images in the hot dtype, every element written.  parts: caller-owned fp32 scratch,
 * ceil(NF / 16) * wgs slabs of sr_mv_recon_slab() floats, one per workgroup, summed in a fixed order (no atomics) into
 * grads = dW_fusion (2F,2F) | db_fusion (2F) | dW_last (2F,3,5,5) | db_last (3), fp32.  1 <= wgs <= 1024. */
int sr_mv_recon_bwd(const void* const* feat_b, const void* const* feat_f, const void* u_save, const float* g, long g_bs, long g_fs,
                    const void* blob, void* const* dfeat_b, void* const* dfeat_f, float* parts, int wgs, float* grads, int F, int NF,
                    int B, int H, int W, int dtype, sr_stream_t stream);
int sr_mv_recon_slab(void);
/* Backward of sr_mv_recon_fwd at cw = 64 (24 < F <= 64): the argument list and the contract of sr_mv_recon_bwd, with
 * u_save = the forward's [NF,B,H,W,128] image, dfeat_b / dfeat_f = [B,H,W,64] images (channels >= F come back exactly zero),
 * blob = packing.mv_recon_bwd_tables(F) (wlb | wfut, the hot dtype) and slabs of sr_mv_recon_slab64() floats.  The slab offset of
 * gradient element i is packing.mv_recon_bwd_tables(F)["reduce"][i].  Frames go 16 per launch; every pointer and size is validated
 * before the first launch: -2 (F outside 25..64, wgs outside 1..1024, a null pointer, g_fs < 48 H W, g_bs < g_fs, more than
 * 2^31 - 1 items per chunk) leaves every buffer untouched.  Added without a change of sr_abi_version(). */
int sr_mv_recon_bwd64(const void* const* feat_b, const void* const* feat_f, const void* u_save, const float* g, long g_bs, long g_fs,
                      const void* blob, void* const* dfeat_b, void* const* dfeat_f, float* parts, int wgs, float* grads, int F, int NF,
                      int B, int H, int W, int dtype, sr_stream_t stream);
int sr_mv_recon_slab64(void);

/* ------------------------------------------------------------------------------------------------
 * Searched network (Result_Model, the NAS stage-3 trainer; csrc/result_block.h).  Activations NHWC in F in {24, 32}
 * channels, the searched width IN <= F first and the rest held at zero.  K in {3, 5, 7}.  Packed weights: packing.rm_conv_frags
 * (rows = output channels in 32-row tiles, k = tap * CI + ci).  mask: one uint32 per pixel, bit c = (conv_k(x) + b)_c > 0.
 * ------------------------------------------------------------------------------------------------ */
/* y = x + ReLU(conv_K(x) + bias), bias float[32]; writes mask.  Weights outside the channel window are zero. */
int sr_rm_block_fwd(const void* x, void* y, unsigned* mask, const void* wp, const float* bias, int N, int H, int W, int F, int K,
                    int dtype, sr_stream_t stream);
/* dx = dy + conv_K^T(dy * mask); wpt = the transposed, flipped weights packed the same way. */
int sr_rm_block_bwd_data(const void* dy, const unsigned* mask, void* dx, const void* wpt, int N, int H, int W, int F, int K,
                         int dtype, sr_stream_t stream);
/* Weight and bias gradient slabs: g [N,H,W,CA] (times mask when mask != NULL: the block), xin [N,H,W,CB] (CB = F).
 * Block: CA = F, K in {3,5,7}.  Tail: mask NULL, CA in {16, 32, 48} (the un-shuffled HR gradient), K in {5, 7}.
 * Grid (wgs, NG): partial[NG][wgs][32 tiles][1024] floats, NG = ceil(ceil(CA / 32) (K^2 + 1) / 32); tile t = 32 g + j of
 * group g is (row tile t / (K^2 + 1), tap t % (K^2 + 1)), tap K^2 = the bias (packing.rm_wgrad_index).  The caller sums wgs. */
int sr_rm_wgrad(const void* g, const unsigned* mask, const void* xin, float* partial, int wgs, int N, int H, int W, int CA, int CB,
                int K, int dtype, sr_stream_t stream);
/* Tail conv with kernel K in {5, 7}: out (NCHW fp32 [N,3,R H,R W], already holding skip + bias from sr_tail_fwd with zero
 * 3x3 weights) += PixelShuffle_R(conv_K(feat)). */
int sr_rm_tail_fwd(const void* feat, float* out, const void* wp, int N, int H, int W, int F, int R, int K, int dtype,
                   sr_stream_t stream);
/* dconv [N,H,W,CP] (CP = 16, 32, 48 for R = 2, 3, 4) = the HR gradient un-shuffled, zero past 3 R^2. */
int sr_rm_unshuffle(const float* dout, void* dconv, int N, int H, int W, int R, int dtype, sr_stream_t stream);
/* dfeat [N,H,W,F] = conv_K^T(dconv); wpt packed from the transposed, flipped tail weights (rows F, CI = CP). */
int sr_rm_tail_bwd_data(const void* dconv, void* dfeat, const void* wpt, int N, int H, int W, int F, int R, int K, int dtype,
                        sr_stream_t stream);

/* Training patches cut on device from a resident uint8 cache.  Replaces, per patch,
 * ImageSuperResolutionDataset._sample_patch + _augment + to_tensor, datasets/_isr.py:68-121.  cache: every LR and HR image
 * as PIL lays them out (H x W x 3 uint8), back to back; recs[B]: one record per patch, drawn on the host in the
 * reference's RNG order; lr_out [B][3][P][P], hr_out [B][3][P*scale][P*scale] fp32 in [0, 1] (either may be NULL). */
typedef struct sr_patch_rec {
  long lr_off, hr_off;      /* byte offsets of the two images in the cache */
  int lr_w, hr_w;           /* their widths in pixels */
  int x, y;                 /* LR crop origin: row x, column y (the reference's names) */
  int flags;                /* 1: flip rows, 2: flip columns, 4: swap axes -- applied in this order */
  int pad_;
} sr_patch_rec_t;
int sr_patch_gather(const unsigned char* cache, const void* recs, float* lr_out, float* hr_out, int B, int P, int scale,
                    sr_stream_t stream);

/* MATLAB-compatible bicubic downscale of uint8 images on device: third_party/matlab_imresize/imresize.py:104-136
 * `imresize(I, scalar_scale=1/scale)` for uint8 input (antialiased cubic, rows then columns, float64 sums in tap order,
 * clipped and rounded half to even back to uint8 after each pass), bit for bit.  wr / ir [ceil(H/scale)][taps_r] and
 * wc / ic [ceil(W/scale)][taps_c]: the weights (float64) and reflected source indices (int32) of the two passes, as
 * packing.bicubic_tables(H or W, scale) builds them; taps <= 18.  img [H][W][3]; out_u8 [ceil(H/scale)][ceil(W/scale)][3];
 * out_f32 [3][ceil(H/scale)][ceil(W/scale)] = the same values / 255 (to_tensor); either output may be NULL, not both.
 * src_f32 (may be NULL) [3][H][W] = the source image / 255: with out_f32 the two sides of an EVAL-mode item from one launch.
 * -1: scale outside {2, 3, 4}; -2: null image or tables, no output, bad sizes or tap counts. */
int sr_bicubic_resize_u8(const unsigned char* img, unsigned char* out_u8, float* out_f32, float* src_f32, int H, int W, int scale,
                         const double* wr, const int* ir, int taps_r, const double* wc, const int* ic, int taps_c,
                         sr_stream_t stream);

/* Bicubic-on-the-fly training batch from a resident HR-only uint8 cache.  Replaces, per patch, TRAIN-mode
 * ImageSuperResolutionBicubicDataset._sample_patch (datasets/_isr.py:197-214) + _augment + to_tensor: the HR crop is the
 * square of side S = (P + 2 ig) scale at row x, column y of its image; it is resized to (P + 2 ig)^2 (the taps reflect at
 * the crop's edges) and the centre P x P is the LR patch; the centre (P scale)^2 of the crop is the HR patch.
 * recs[B]: one record per patch, drawn on the host in the reference's RNG order; w / idx [P + 2 ig][taps]:
 * packing.bicubic_tables(S, scale), one pair for the whole batch; lr_out [B][3][P][P], hr_out [B][3][P*scale][P*scale]
 * fp32 in [0, 1] (either may be NULL).  -1: scale outside {2, 3, 4}; -2: ig < 1, null tables, B > 65535, ... */
typedef struct sr_bicubic_rec {
  long hr_off;              /* byte offset of the HR image in the cache */
  int hr_w;                 /* its width in pixels */
  int x, y;                 /* HR crop origin: row x, column y (the reference's names) */
  int flags;                /* 1: flip rows, 2: flip columns, 4: swap axes -- applied in this order */
} sr_bicubic_rec_t;
int sr_bicubic_patch_gather(const unsigned char* cache, const void* recs, float* lr_out, float* hr_out, int B, int P, int scale,
                            int ig, const double* w, const int* idx, int taps, sr_stream_t stream);

/* Video training clips cut on device from a resident frame cache.  Replaces, per clip item in TRAIN mode,
 * the `__getitem__` of VideoSuperResolution(Hdf5)Dataset / VideoSuperResolutionWithMVHdf5Dataset: `_sample_patch`, `to_tensor`,
 * the stack over frames and `_augment`, datasets/_vsr.py:59-180, :314-432.  cache: every LR and HR frame (H x W x 3 uint8) back
 * to back, followed by at least 16 bytes of padding (runs are read with wide loads); mv_cache (NULL: RGB items): every motion
 * vector frame (H x W x 2 float32, the LR frame's H x W), 8-byte aligned; frames[]: one entry per frame; ids[]: the frame ids
 * of every clip; recs[B]: one record per item, drawn on the host in the reference's RNG order.  Every frame of item b is cut
 * at the same window.  lr_out [B][T][C][P][P] fp32, C = 3 (RGB / 255) or 5 with mv_cache (channels 3, 4: the motion vector,
 * not scaled); hr_out [B][T][3][P*scale][P*scale] fp32 in [0, 1]; either may be NULL (lr_out not with mv_cache).
 * B * T <= 65535, P * scale <= 8192, lr_out / hr_out 16-byte aligned. */
typedef struct sr_clip_rec {
  long ids_off;             /* position of the clip's first frame id in ids[] */
  int x, y;                 /* LR crop origin: row x, column y (the reference's names) */
  int flags;                /* 1: reverse the width (p1 < 0.5), 2: reverse the height (p2 < 0.5) */
  int T;                    /* number of frame ids of the clip (frames t >= T are not written) */
} sr_clip_rec_t;
typedef struct sr_clip_frame {
  long lr_off, hr_off;      /* byte offsets of the frame's LR and HR images in cache */
  long mv_off;              /* byte offset of its motion vectors in mv_cache (unused without) */
  int lr_w, hr_w;           /* widths in pixels */
} sr_clip_frame_t;
int sr_clip_gather(const unsigned char* cache, const float* mv_cache, const void* frames, const int* ids, const void* recs,
                   float* lr_out, float* hr_out, int B, int T, int P, int scale, sr_stream_t stream);

/* Evaluation metrics on device: psnr (luma = 0; common/metrics.py:10-19: 8-bit quantised sr) and psnr_y (luma = 1 for
 * 3-channel images; :22-38: clamped but NOT quantised -- the reference drops its quantised copy -- with the luma filter
 * on the difference; luma = -1: the same without the filter, what the reference does when dim 1 is not 3).  sr, hr
 * [N][C][H][W] fp32; partial [N * wgs] scratch; out[0] = sum over the batch of -10 log10(mse) (the reference sums). */
int sr_psnr(const float* sr, const float* hr, float* partial, float* out, int N, int C, int H, int W, int shave, int luma,
            int wgs, sr_stream_t stream);

/* ssim of the evaluation loop on device (common/metrics.py:41-68: skimage's structural_similarity, 11 x 11 Gaussian window
 * of sigma 1.5, data_range 1, sample covariance, on the fp32 lumas of the 8-bit quantised sr and of hr, both shaved; from
 * the filter on in double).  sr, hr [N][3][H][W] fp32; partial: scratch of n_partial doubles, at least
 * N * ceil((H - 2 shave - 10) / 32) * ceil((W - 2 shave - 10) / 32) (one per 32 x 32 tile of output pixels);
 * out[0] = sum over the batch of the per-image mean (one image: the reference's value).  No atomics: the same input gives
 * the same bits.  -2: null pointer, N <= 0 or > 65535, shave < 1, H - 2 shave < 11 or W - 2 shave < 11, partial too small. */
int sr_ssim(const float* sr, const float* hr, double* partial, double* out, int N, int H, int W, int shave, long n_partial,
            sr_stream_t stream);

/* The evaluation loops' per-frame epilogue on device (utils/estimate.py:70-104, test_video_superresolution_by_patch.py:
 * 198-224).  sr, hr [F][3][H][W] fp32, lr [F][lr_channels][h][w] fp32 (channels 0..2 used: `baseline[:, :3]`).  The
 * bilinear baseline interpolate(lr, (H, W), mode='bilinear', align_corners=...) is ATen's upsample_bilinear2d in fp32,
 * blended in registers and never stored.  out [4][F] fp32, per frame: psnr(sr, hr), psnr_y(sr, hr), psnr(baseline, hr)
 * with `shave` (nan when nothing is left, as sr_psnr), and the Charbonnier mean sqrt((sr - hr)^2 + 1e-12) over the
 * UNSHAVED frame.  partial: scratch of F * wgs * 4 floats, 16-byte aligned; wgs workgroups per frame (1..65535).
 * -2: null pointer, F outside 1..65535, a side outside 1..32768, lr_channels < 3, shave < 0, partial misaligned. */
int sr_eval_clip(const float* sr, const float* lr, const float* hr, float* partial, float* out, int F, int H, int W, int h,
                 int w, int lr_channels, int shave, int align_corners, int wgs, sr_stream_t stream);

/* 8-bit frames as torchvision's save_image quantises them: uint8(clamp(clamp(x, 0, 1) * 255 + 0.5, 0, 255)) in fp32,
 * NCHW fp32 -> out [F][H][W][3] uint8 (4-byte aligned).  from_lr = 0: src [F][3][H][W] (src_channels must be 3; h, w
 * unused); from_lr = 1: src [F][src_channels][h][w], the bilinear baseline of its first three channels at (H, W) as in
 * sr_eval_clip, never stored in float. */
int sr_eval_u8(const float* src, unsigned char* out, int F, int H, int W, int h, int w, int src_channels, int from_lr,
               int align_corners, sr_stream_t stream);

/* total_variation and time_variation of test_video_superresolution_by_patch.py:43-69 per frame of lr [B][N][C][h][w]
 * fp32: out [2][B * N] fp32, row 0 = sum |down - x| + |right - x| with the last row and column replicated, row 1 = the sums
 * of |x[n + 1] - x[n]| of a frame's one or two neighbours, doubled for the first and the last frame of a clip (zeros for
 * N = 1).  partial: scratch of B * N * wgs * 2 floats.  -2: null pointer, B * N outside 1..65535, C * h * w > 2^30. */
int sr_eval_variation(const float* lr, float* partial, float* out, int B, int N, int C, int h, int w, int wgs,
                      sr_stream_t stream);

/* flow_warp, models/spynet_arch.py:98-129 (bilinear, zeros padding, align_corners=True): x, out NCHW fp32;
 * flow (N,H,W,2).  Backward: dx (zero-filled by the caller, may be NULL) and dflow (may be NULL). */
int sr_flow_warp_fwd(const float* x, const float* flow, float* out, int N, int C, int H, int W, sr_stream_t stream);
int sr_flow_warp_bwd(const float* x, const float* flow, const float* gout, float* dx, float* dflow, int N, int C,
                     int H, int W, sr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * NAS supernet block: Split_Block.forward_body (models/wdsr_b.py:482-496) with Conv_sep branches
 * (:375-402), the BinaryConv2d masks (models/ops.py:7-43) and the hard skip/keep gate of
 * MyAggregationLayer.forward (:517-546):  y = mg*yin + beta2 * ms * sum_k p_k relu(pw_k(relu(dw_k(mg*ms*yin)))).
 * Tables/fragments: mobilesuperresolution_amd/packing.py nas_tables().  V / GZ: [3][N][H][W][F].
 * ------------------------------------------------------------------------------------------------ */
int sr_nas_dw_fwd(const void* yin, void* V, const float* dwp, int N, int H, int W, int F, int dtype, sr_stream_t stream);
int sr_nas_pw_fwd(const void* yin, const void* V, void* y, const void* frags, const float* tabs, const float* scal,
                  int N, int H, int W, int F, int dtype, sr_stream_t stream);
/* partial[wgs][3*(1024+64)+4]: per branch dWpw tile | dbp[32] | r[32]; then sum(gy*mg*yin). */
int sr_nas_pw_bwd(const void* yin, const void* V, const void* gy, void* GZ, const void* frags, const float* tabs,
                  const float* scal, float* partial, int wgs, int N, int H, int W, int F, int dtype,
                  sr_stream_t stream);
/* partial[wgs][88*32]: dWdw[83 taps][32] | dbd[3][32] | sum(g_br*mg*yin)[32] | sum(g_x*yin)[32]. */
int sr_nas_dw_bwd(const void* yin, const void* GZ, const void* gy, void* gyin, const float* dwp, float* partial,
                  int wgs, int N, int H, int W, int F, int dtype, sr_stream_t stream);
/* Depthwise weight gradients dWdw[83 taps][32] of the same slab (same `wgs`), on the matrix cores; call after
 * sr_nas_dw_bwd on the same stream (it fills the part of each slab that sr_nas_dw_bwd leaves untouched). */
int sr_nas_dw_wgrad(const void* yin, const void* GZ, const float* dwp, float* partial, int wgs, int N, int H, int W,
                    int F, int dtype, sr_stream_t stream);

/* Every block of the supernet body from one call each way (the per-op entry points above, looped in C: 2 launches per
 * block forward, 3 backward).  ys [(nb+1)][N][H][W][F] (slot 0 = input, slot nb = output); V [nb][3][N][H][W][F];
 * per-block tables at BYTE strides: dwp (dwp_bs), frags (frags_bs), tabs (tabs_bs), scal (scal_bs).  Backward: g_out =
 * gradient at ys[nb]; g_tmp[2] two activation-sized scratch buffers; GZ [3][N][H][W][F] scratch; part_pw / part_dw
 * [nb][wgs][slab] at byte strides pw_bs / dw_bs.  *g_in receives the pointer (g_tmp[0] or g_tmp[1]) that holds the gradient at ys[0].
 * bf16 at F = 24 / 32 fuses a block's two forward kernels into one launch, and its backward's pointwise and depthwise-weight
 * kernels when N x tiles <= wgs; split != 0 keeps the separate kernels (the parity tests compare the two routes). */
/* 0/1 masks, gates and latency terms of a supernet step, values only (models/ops.py:33-43, wdsr_b.py:517-534,
 * speed_estimator.py:57-76).  split_w (nb, F), alpha (nb, 3), alpha1 / alpha2 (nb).
 * out: mask_hard[F] | c_mask | ms_hard[nb][F] | c_split[nb] | speed_curr[nb] | gates[nb][2]  (F + 1 + nb (F + 4) floats).
 * One workgroup; -1 if (nb + 1) F > 4096. */
int sr_nas_scalars(const float* mask_w, const float* split_w, const float* alpha, const float* alpha1, const float* alpha2,
                   int nb, int F, float* out, float* src, long src_stride, int off_mg, float* scal, sr_stream_t stream);
/* optional outputs of sr_nas_scalars (NULL: skipped): `src` -- the mask columns mg | ms | mg ms | 0 | 1 (3 F + 2 floats at column
 * off_mg) of nb operand-source rows of src_stride floats (sr_param_pack gathers them); `scal` -- nb x {softmax(alpha)[3], gate2}.
 * sr_nas_mask_grads: the gradients of the masks / gates / branch weights from the sums the block kernels left in d(source)
 * (columns off_r: r[3][F], off_sxy, off_sA: [F], off_sB: [F] of rows of `ds` floats), ms (nb, F), p (nb, 3), beta (nb, 2):
 * out = g_p[nb][3] | g_beta[nb][2] | g_ms[nb][F] | g_mg[F]   (wdsr_b.py:517-546 differentiated) */
int sr_nas_mask_grads(const float* dsrc, long ds, int off_r, int off_sxy, int off_sA, int off_sB, const float* ms, const float* p,
                      const float* beta, int nb, int F, float* out, sr_stream_t stream);
int sr_nas_body_fwd(void* ys, void* V, const float* dwp, long dwp_bs, const void* frags, long frags_bs, const float* tabs,
                    long tabs_bs, const float* scal, long scal_bs, int nb, int N, int H, int W, int F, int dtype,
                    int split, sr_stream_t stream);
int sr_nas_body_bwd(const void* ys, const void* V, const void* g_out, void* g_tmp0, void* g_tmp1, void* GZ, const float* dwp,
                    long dwp_bs, const void* frags, long frags_bs, const float* tabs, long tabs_bs, const float* scal,
                    long scal_bs, float* part_pw, long pw_bs, float* part_dw, long dw_bs, int wgs, int nb, int N, int H, int W,
                    int F, int dtype, int split, void** g_in, sr_stream_t stream);

/* Parameter plumbing of a table-described model (the supernet body; the same kernels sr_wdsr_net_forward / _backward run on
 * BASIC_MODEL's tables): weight-norm of the flat fp32 parameters into `src` (reference: torch.nn.utils.weight_norm around
 * every conv, models/wdsr_b.py:375-402), then up to four gathers of `src` into the packed operand tables the compute
 * kernels read; and the way back: workgroup slabs summed and scattered into `dsrc` (laid out like `src`, plus whatever extra
 * columns the tables name), then the weight-norm backward into `gflat` (laid out like `flat`; entries no table row names are
 * left untouched).  chan_tab: int[n_chan][4] = {v_off, g_off, K, dst_off}; bias_tab: int[n_bias][3] = {src_a, src_b | -1, dst}. */
typedef struct { const int* idx; void* out; long src_off, src_stride; int n, reps, as_float; } sr_pack_seg_t;
typedef struct { const float* partial; const int* sidx; const int* dst; long dst_off, dst_stride, slab; int wgs, n, reps; } sr_unpack_seg_t;
int sr_param_pack(const float* flat, float* src, const int* chan_tab, int n_chan, const int* bias_tab, const float* bias_const,
                  int n_bias, const sr_pack_seg_t* segs, int nseg, int dtype, sr_stream_t stream);
int sr_param_grads(const float* flat, float* dsrc, float* gflat, const int* chan_tab, int n_chan, const int* bias_tab,
                   int n_bias, const sr_unpack_seg_t* segs, int nseg, sr_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Whole-network entry points: everything BASIC_MODEL.forward (models/basic_wdsr_b.py:85-93) and its
 * autograd backward do, as ONE call each.  The caller (mobilesuperresolution_amd/models) owns every
 * buffer; `sr_wdsr_net_t` only carries device pointers, table sizes and the geometry.
 * Parameters live in one flat fp32 buffer (layout: mobilesuperresolution_amd/layout.py).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
  int F, NB, R, dtype, N, H, W;
  float mean;
  /* parameters, their gradient, weight-norm tables */
  const float* flat; float* gflat;
  const int* chan_tab; int n_chan;              /* int4 {v_off, g_off, K, dst_off} per output channel */
  const int* bias_tab; const float* bias_const; int n_bias;   /* int3 {src_a, src_b, dst} per bias element */
  /* canonical effective-weight vectors (src) and their gradient (dsrc): head | body[NB] | tail */
  float* src; float* dsrc;
  long src_head_off, src_body_off, src_body_stride, src_tail_off;
  /* fragment packing tables and packed blobs */
  const int* idx_head; int n_idx_head;
  const int* idx_body; int n_idx_body;
  const int* idx_cinit; int n_idx_cinit;
  const int* idx_tail; int n_idx_tail;
  void* blob_head; void* blob_body; float* cinit_body; void* blob_tail;
  /* gradient slabs written by the weight-gradient kernels and their gather tables {slab idx, dst idx} */
  float* part_a; float* part_b; float* part_tail; float* part_head;
  int wgs_body, wgs_tail, wgs_head;
  int slab_a, slab_b, slab_tail, slab_head;
  const int* ga_sidx; const int* ga_dst; int n_ga;
  const int* gb_sidx; const int* gb_dst; int n_gb;
  const int* gt_sidx; const int* gt_dst; int n_gt;
  const int* gh_sidx; const int* gh_dst; int n_gh;
  /* activations: x NCHW fp32; acts/grads [(NB+1)][N][H][W][F] (acts may be 2 ping-pong slots when
   * save_acts == 0); out / dout NCHW fp32 [N][3][R*H][R*W] */
  const float* x; void* acts; void* grads; float* out; const float* dout;
  /* optional (bf16; NULL = recompute in backward): t and dt of every block, [NB][N][tiles][288][LP] */
  void* tsave; void* dtsave;
  /* optional loss fold (hr != NULL): backward reads `out` and `hr` (NCHW fp32 HR target) instead of `dout` and forms
   * the L1 (loss_kind 1, pretrain.py:73) or Charbonnier (2, train_video_superresolution.py:43-53) gradient on the
   * fly, loss_gscale = upstream gradient / numel; loss_part[wgs_tail] receives the per-workgroup loss sums */
  const float* hr; int loss_kind; float loss_gscale; float* loss_part;
  /* optional two-part backward (sr_wdsr_net_backward_part): first block of the late half, and the rows of chan_tab /
   * bias_tab where the late parameters (body[nb_split..], tail, skip) begin */
  int nb_split, chan_split, bias_split;
  /* sr_wdsr_net_train_step only: 1 = every parameter belongs to exactly one row of chan_tab / bias_tab, so the Adam update is
   * applied by the weight-norm backward's launch (one launch less); 0 = separate sr_adam_step pass */
  int adam_in_wn_bwd;
  /* 32 units, bf16: 1 = one block per launch where the network would run two (forward and backward alike) */
  int one_block32;
} sr_wdsr_net_t;

/* weight-norm + packing + head + NB fused blocks + fused tail.  flags: SR_NET_SAVE_ACTS keeps every block input
 * (needed by sr_wdsr_net_backward), otherwise two slots ping-pong (inference); SR_NET_WEIGHTS_PACKED skips the
 * weight-norm + packing launches (the caller guarantees the packed blobs in `net` are those of `flat`, e.g. repeated
 * inference with unchanged parameters). */
#define SR_NET_SAVE_ACTS 1
#define SR_NET_WEIGHTS_PACKED 2
#define SR_NET_PACK_ONLY 4   /* weight-norm + packing of `flat` into the blobs, nothing else (backward after the blobs were re-packed) */
#define SR_NET_SKIP_TAIL 8   /* stop after the last block: acts[NB] is written, `out` is not (the caller runs sr_tail_train next) */
int sr_wdsr_net_forward(const sr_wdsr_net_t* net, int flags, sr_stream_t stream);
/* full backward: d(loss)/d(out) -> gflat (gradient of every parameter in the flat buffer). */
int sr_wdsr_net_backward(const sr_wdsr_net_t* net, sr_stream_t stream);
/* The same in two parts, so that a data-parallel trainer can all-reduce the late parameters' gradient while the early
 * half of the backward still runs (pretrain.py:239 DDP overlap): part 1 = tail + blocks [nb_split, NB) (their entries
 * of gflat are final on return), part 2 = blocks [0, nb_split) + head; part 0 = everything. */
int sr_wdsr_net_backward_part(const sr_wdsr_net_t* net, int part, sr_stream_t stream);

/* Standalone nn.PixelShuffle(r) (models/basic_wdsr_b.py:80-83; basicvsr_arch_origin.py:37,87-88), NCHW fp32, bit-exact:
 * out[n, c, h r + i, w r + j] = in[n, c r^2 + i r + j, h, w].  C = channels of the shuffled tensor, H x W = size before
 * the shuffle.  inverse != 0 runs the inverse permutation (pixel_unshuffle = the op's backward): in is then the
 * N x C x rH x rW tensor and out the N x C r^2 x H x W one. */
int sr_pixel_shuffle(const float* in, float* out, int N, int C, int H, int W, int r, int inverse, sr_stream_t stream);

/* Tail backward with the loss folded in (see sr_wdsr_net_t.hr): sr = network output, hr = target. */
int sr_tail_bwd_loss(const float* sr, const float* hr, int loss_kind, float gscale, float* loss_part, const void* feat,
                     const float* x_nchw, float mean, const void* wblob, void* dfeat, float* partial, int wgs, int N, int H,
                     int W, int F, int R, int dtype, sr_stream_t stream);

/* Tail forward + folded loss + tail backward in ONE launch, for the training step: writes what sr_tail_fwd followed by
 * sr_tail_bwd_loss writes to dfeat, partial and loss_part, bit for bit; the SR image is never stored.  bf16, R = 4,
 * F = 24 or 32 (-1 otherwise). */
int sr_tail_train(const float* hr, int loss_kind, float gscale, float* loss_part, const void* feat, const float* x_nchw, float mean,
                  const void* wblob, void* dfeat, float* partial, int wgs, int N, int H, int W, int F, int R, int dtype,
                  sr_stream_t stream);

/* One Adam step over a flat fp32 parameter buffer with the arithmetic of torch.optim.Adam's default (foreach)
 * implementation (pretrain.py:137: lr 1e-3 x world, betas (0.9, 0.999), eps 1e-8, no weight decay).  The caller
 * computes the step-dependent scalars in double and rounds them to float, as torch does:
 *   w_lerp = 1 - beta1, one_minus_beta2 = 1 - beta2, bc2_sqrt = sqrt(1 - beta2^t), neg_step_size = -lr / (1 - beta1^t).
 * loss_out (may be NULL) = loss_scale * sum(loss_part[0 .. n_loss)). */
typedef struct { float w_lerp, beta2, one_minus_beta2, bc2_sqrt, eps, neg_step_size; } sr_adam_t;
int sr_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, const sr_adam_t* a,
                 const float* loss_part, int n_loss, float loss_scale, float* loss_out, sr_stream_t stream);
/* The same step for `count` tensors in ONE launch: 1 <= count <= SR_ADAM_MULTI_CAP rows {param, grad, exp_avg, exp_avg_sq, n >= 1},
 * all contiguous fp32 device buffers; `rows` is a HOST array, copied into the kernel's arguments (gradient pointers change every step
 * under zero_grad(set_to_none=True), a table cached on the device would go stale).  The capacity follows from HIP's 4096 bytes of
 * kernel arguments: 80 rows x 48 bytes + the scalars.  Workgroups map to (tensor, chunk of SR_ADAM_MULTI_CHUNK elements); the
 * arithmetic per element is sr_adam_step's, bit for bit.  No loss fold.  -2 = invalid arguments (count outside the range included),
 * -1 = more than 2^31 - 1 chunks.  Added without a change of sr_abi_version(). */
#define SR_ADAM_MULTI_CAP 80
#define SR_ADAM_MULTI_CHUNK 1024
typedef struct { float* param; const float* grad; float* exp_avg; float* exp_avg_sq; long n; } sr_adam_row_t;
int sr_adam_step_multi(const sr_adam_row_t* rows, int count, const sr_adam_t* a, sr_stream_t stream);
int sr_loss_value(const float* loss_part, int n_loss, float loss_scale, float* loss_out, sr_stream_t stream);
/* y[i] = x[i] * (*scale), the product in fp32; x, y: n elements of `dtype`, 16-byte aligned; scale: a device scalar.  What
   `loss_weight * criterion(sr, hr)` (search.py:74, pretrain.py:73) makes of a folded loss's data gradient: autograd hands the
   weight over as a device tensor, torch's own multiply would round it to the gradient's dtype first. */
int sr_scale_by(void* y, const void* x, long n, const float* scale, int dtype, sr_stream_t stream);
/* forward + loss-folded backward + Adam in one call (net->hr etc. set; net->flat is updated in place). */
int sr_wdsr_net_train_step(const sr_wdsr_net_t* net, float* exp_avg, float* exp_avg_sq, long n_params, const sr_adam_t* a,
                           float loss_scale, float* loss_out, sr_stream_t stream);

/* ---- SPyNet's 7x7 convolutions (models/spynet_arch.py:17-22), bf16 activations NHWC ----
 * y[n, h, w, co] = act(bias[co] + sum_{ky, kx, ci} w[co, ci, ky, kx] x[n, h + ky - 3, w + kx - 3, ci]), zero padding.
 * x: [N][H][W][CIN] bf16; wpacked: the layer's weights as MFMA fragments [7 ky][k-step][32-row tile][64 lanes][8] bf16 (k-step =
 * (kx, 16 input channels), for CIN = 8: two adjacent taps; packing.conv7_pack builds it); bias: [ceil(COUT / 32) * 32] fp32;
 * y: [N][H][W][COUT] bf16, or fp32 when out_f32.  Supported (CIN, COUT, relu, out_f32): (8,32,1,0) (32,64,1,0) (64,32,1,0)
 * (32,16,1,0) (16,2,0,1) -- the five layers of a BasicModule; anything else returns -1. */
int sr_conv7_fwd(const void* x, const void* wpacked, const float* bias, void* y, int N, int H, int W, int CIN, int COUT, int relu,
                 int out_f32, sr_stream_t stream);

/* ---- SPyNet's 7x7 convolutions, backward (SpyNet.hot_training; added without a change of sr_abi_version()) ----
 * CIN, COUT name the FORWARD layer, one of the five above; anything else returns -1, a missing buffer -2, and nothing is written.
 * Backward-data: dx = mask * conv7(dy, rot180(w) with the channel roles swapped), no bias.  dy: [N][H][W][max(COUT, 8)] bf16 (the
 * last layer's two-channel flow gradient zero-padded to 8 channels); wpacked_t: packing.conv7_bwd_tables' fragments, bf16;
 * act: [N][H][W][CIN] bf16, the layer's saved input -- dx is multiplied by act > 0 and stored [N][H][W][CIN] in bf16.  CIN = 8
 * (first layer): act is ignored and dx is fp32, unmasked. */
int sr_conv7_bwd_data(const void* dy, const void* wpacked_t, const void* act, void* dx, int N, int H, int W, int CIN, int COUT,
                      sr_stream_t stream);
/* Weight and bias gradient: gflat[COUT * CIN * 49 + COUT] = dW (COUT, CIN, 7, 7) | db, fp32, every element written once.  dy as
 * above, x: [N][H][W][CIN] bf16.  partial: wgs slabs of packing.conv7_wgrad_tables(CIN, COUT)["slab"] floats: workgroup w walks the
 * 16 x 16 pixel tiles w, w + wgs, .. and writes slab w; one reduction launch sums the slabs in slab order through sidx / dst (the
 * same tables, device int arrays of COUT * CIN * 49 + COUT entries).  No float atomics: equal calls give equal bits. */
int sr_conv7_wgrad(const void* dy, const void* x, float* partial, int wgs, const int* sidx, const int* dst, float* gflat, int N,
                   int H, int W, int CIN, int COUT, sr_stream_t stream);
/* The backward of one BasicModule call in one C call.  x[l]: layer l's saved input; g[l]: the gradient at layer l's output (g[4]
 * filled by the caller, g[0..3] written: g[l - 1] = dx_l); dx0: [N][H][W][8] fp32; partial: wgs slabs of the largest layer. */
typedef struct {
  const void* x[5];
  void* g[5];
  const void* wpacked_t[5];
  const int* sidx[5];
  const int* dst[5];
  float* gflat[5];
  float* partial;
  void* dx0;
} sr_conv7_module_bwd_t;
int sr_conv7_module_bwd(const sr_conv7_module_bwd_t* m, int wgs, int N, int H, int W, sr_stream_t stream);

/* ---- per-frame video network (models/single_image_model.py Result_Model), inference (csrc/frame_net.h) ----
 * frames: fp32 [N,3,H,W] (N = clips x frames); blob: packing.fn_tables layout in `dtype`, conv_off: HOST array of 2 nb + 2 element
 * offsets into it (block i: conv_off[2 i] with its second conv right behind it, the body's last conv: conv_off[2 nb], the upsampler:
 * conv_off[2 nb + 1]); head_blob: packing.ends_tables(32, 4)["head"] of the encoder padded to 32 rows.  s0, s1, s2: caller-owned
 * [N,H,W,32] scratch images in `dtype`: s0 = e, the blocks alternate s1, s2, s1, .., the last conv writes f into the one of s1 / s2 that
 * its input is not.  out: image n at out + n * out_is, NCHW fp32 (3, 4H, 4W), or with SR_FN_WRITE_D the transposed conv's own
 * (3, 4H + 1, 4W + 1) output.  stages: which layers run, each on the scratch as it stands.  Allocates nothing, never synchronises;
 * -1 = unsupported geometry (N > 65535, H or W > 8192, nb > 1024, dtype), every buffer untouched. */
#define SR_FN_ENCODER 1
#define SR_FN_BLOCKS 2
#define SR_FN_LAST 4
#define SR_FN_UP 8
#define SR_FN_WRITE_D 16
#define SR_FN_ALL 15
int sr_fn_net_fwd(const float* frames, const void* blob, const long* conv_off, const void* head_blob, void* s0, void* s1, void* s2,
                  float* out, long out_is, int nb, int N, int H, int W, int dtype, int stages, sr_stream_t stream);

/* ---- per-frame video network, the training route (csrc/frame_net.h, csrc/frame_net_bwd.h, csrc/result_block.h) ----
 * sr_fn_net_train_fwd is sr_fn_net_fwd (same kernels, bit-identical out) that keeps what the backward reads, all caller-owned, images
 * [N,H,W,32] in `dtype`: acts = nb + 2 images (acts[0] = e, acts[i] = block i's input, acts[nb] = the last conv's input,
 * acts[nb + 1] = f); ts = nb images (block i's t = ReLU(conv1(x_i))); masks = nb x [N,H,W] uint32 (bit c: conv1's fp32 accumulator of
 * channel c > 0).  ts and masks may be NULL when nb == 0.  stages: SR_FN_ENCODER .. SR_FN_UP (SR_FN_WRITE_D is not accepted).
 *
 * sr_fn_net_bwd: g: d(loss)/d(out), image n at g + n * g_is, NCHW fp32 (3, 4H, 4W); bwd_blob: packing.fn_bwd_tables layout in `dtype`
 * (per conv the 18 rm_conv fragments of W^T with both taps flipped, then the upsampler's 6 backward fragments); gs: 4 scratch
 * images: gs[0] = df, gs[1] = the last conv's input gradient, block i = nb - 1 .. 0 reads its dy from gs[1] / gs[3] and writes dx into
 * the other (so dx_0 ends in gs[1] for even nb, gs[3] for odd), gs[2] = dt and at the end de = dx_0 + df.  parts: fp32 workgroup
 * slabs, (2 nb + 1) x wgs x 32768 (convs) + wgs x 2576 (upsampler) + wgs x 3072 (encoder) floats; 1 <= wgs <= 1024 workgroups walk the
 * tiles of each weight-gradient launch.  grads (fp32, C = the model's channels): conv j's dW (C,C,3,3) | db (C) at j (9 C C + C), then
 * the upsampler's dW (C,3,5,5) | db (3), then the encoder's dW (C,3,3,3) | db (C), every slab summed in workgroup order by one
 * launch; only the sections of the stages that ran are written.  stages: which layers run, each on gs as it stands.  No atomics.
 * Both: allocate nothing, never synchronise; -2 = invalid arguments, -1 = unsupported geometry (as sr_fn_net_fwd, or more than
 * 2^31 - 1 frames x 8 x 16 tiles), every buffer untouched. */
#define SR_FN_BWD_UP 1
#define SR_FN_BWD_LAST 2
#define SR_FN_BWD_BLOCKS 4
#define SR_FN_BWD_ENCODER 8
#define SR_FN_BWD_ALL 15
int sr_fn_net_train_fwd(const float* frames, const void* blob, const long* conv_off, const void* head_blob, void* acts, void* ts,
                        unsigned* masks, float* out, long out_is, int nb, int N, int H, int W, int dtype, int stages,
                        sr_stream_t stream);
int sr_fn_net_bwd(const float* frames, const float* g, long g_is, const void* bwd_blob, const void* acts, const void* ts,
                  const unsigned* masks, void* gs, float* parts, int wgs, float* grads, int C, int nb, int N, int H, int W, int dtype,
                  int stages, sr_stream_t stream);
/* sr_fn_net_bwd with the trainers' loss folded into its first stage (the conventions of sr_tail_bwd_loss): in place of g, sr = the
 * network's output and hr = the target, image n of both at + n * g_is, NCHW fp32 (3, 4H, 4W); loss_kind 1 = L1, 2 = Charbonnier (eps
 * 1e-12); gscale = upstream / sr.numel().  Every gradient value the upsampler's backward would have loaded is formed in registers from
 * sr and hr in fp32 (L1: gscale sign(d), Charbonnier: d / sqrt(d d + eps) gscale, d = sr - hr); no d(loss)/d(sr) tensor exists.
 * loss_part: min(N x ceil(H / 8) x ceil(W / 16), wgs) floats, one per workgroup of that stage: its share of sum |d| resp.
 * sum sqrt(d d + eps), every HR pixel counted once, by the workgroup whose 8 x 16 tile owns it; sr_loss_value sums them.  stages
 * must include SR_FN_BWD_UP.  Everything after the first stage is sr_fn_net_bwd's.  Added without a change of sr_abi_version(). */
int sr_fn_net_bwd_loss(const float* frames, const float* sr, const float* hr, int loss_kind, float gscale, float* loss_part, long g_is,
                       const void* bwd_blob, const void* acts, const void* ts, const unsigned* masks, void* gs, float* parts, int wgs,
                       float* grads, int C, int nb, int N, int H, int W, int dtype, int stages, sr_stream_t stream);

/* ---- per-frame video network, any output size: the three entry points above with the reference's
 * F.interpolate(D, (OH, OW), 'bilinear') inside the upsampler kernels, forward and backward, for any 1 <= OH, OW <= SR_FN_MAX_OUT.
 * out / g: image n at + n * out_is / g_is, NCHW fp32 (3, OH, OW), every element of out written once.  The resize arithmetic is not
 * done on the device: ty, ly (and tx, lx over OW and 4W + 1) are DEVICE tables made on the host by packing.resize_axis(4H + 1, OH):
 * ty = i0 [OH] | lo [4H + 1] | hi [4H + 1] (int32), ly = lam [OH] (fp32); output d blends D rows i0[d] and min(i0[d] + 1, 4H) with
 * 1 - lam[d] and lam[d]; lo[i] .. hi[i] are the outputs with i0 == i (hi = lo - 1: none), which is what the backward gathers over.
 * The tables are trusted as the blobs are.  stages as sr_fn_net_fwd (without SR_FN_WRITE_D), sr_fn_net_train_fwd and sr_fn_net_bwd;
 * everything but the upsampler's resize is theirs, no atomics, equal calls give equal bits.  -2 = invalid arguments (theirs, a NULL
 * table, OH or OW < 1, out_is / g_is < 3 OH OW), -1 = unsupported geometry (theirs, OH or OW > SR_FN_MAX_OUT), every buffer
 * untouched.  Added without a change of sr_abi_version(). */
#define SR_FN_MAX_OUT 32768
int sr_fn_net_fwd_sized(const float* frames, const void* blob, const long* conv_off, const void* head_blob, void* s0, void* s1, void* s2,
                        float* out, long out_is, int OH, int OW, const int* ty, const float* ly, const int* tx, const float* lx, int nb,
                        int N, int H, int W, int dtype, int stages, sr_stream_t stream);
int sr_fn_net_train_fwd_sized(const float* frames, const void* blob, const long* conv_off, const void* head_blob, void* acts, void* ts,
                              unsigned* masks, float* out, long out_is, int OH, int OW, const int* ty, const float* ly, const int* tx,
                              const float* lx, int nb, int N, int H, int W, int dtype, int stages, sr_stream_t stream);
int sr_fn_net_bwd_sized(const float* frames, const float* g, long g_is, int OH, int OW, const int* ty, const float* ly, const int* tx,
                        const float* lx, const void* bwd_blob, const void* acts, const void* ts, const unsigned* masks, void* gs,
                        float* parts, int wgs, float* grads, int C, int nb, int N, int H, int W, int dtype, int stages,
                        sr_stream_t stream);
/* sr_fn_net_bwd_loss at any output size = sr_fn_net_bwd_sized with the loss folded as in sr_fn_net_bwd_loss: sr and hr NCHW fp32
 * (3, OH, OW), image n of both at + n * g_is; gscale = upstream / sr.numel().  The loss terms are collected where the upsampler's
 * backward sums db_up: over the outputs whose source cell (i0_y, i0_x) the workgroup's 8 x 16 tile owns by the forward's rule, every
 * output once.  loss_part: min(N x ceil(H / 8) x ceil(W / 16), wgs) floats, EVERY one written by every call (0 from a workgroup whose
 * tiles own no output, as most do at a downscale).  -2 / -1 as sr_fn_net_bwd_loss and sr_fn_net_bwd_sized together, every buffer
 * untouched.  Added without a change of sr_abi_version(). */
int sr_fn_net_bwd_loss_sized(const float* frames, const float* sr, const float* hr, int loss_kind, float gscale, float* loss_part,
                             long g_is, int OH, int OW, const int* ty, const float* ly, const int* tx, const float* lx,
                             const void* bwd_blob, const void* acts, const void* ts, const unsigned* masks, void* gs, float* parts,
                             int wgs, float* grads, int C, int nb, int N, int H, int W, int dtype, int stages, sr_stream_t stream);

/* ---- multi-frame video network (models/naive_multi_model_easy.py Naive_model), inference (csrc/multi_frame.h) ----
 * frames: fp32 [B N,3,H,W] (clip b's frame i at index b N + i); flows: fp32 [B,N-1,2,H,W], channel 0 = dx, the flow that warps frame
 * i - 1's features onto frame i at index i - 1 (NULL allowed when N == 1); blob: packing.mf_tables layout in `dtype` (block 0, blocks
 * 1 .. nb - 1 as per-frame-network blocks, the decode conv; the offsets follow from nb); head_blob: the encoder as for sr_fn_net_fwd.
 * s0, s1, s2: caller-owned [B N,H,W,32] scratch images in `dtype`: s0 = e (all frames stay live for the warp), block 0 writes s1, the
 * blocks alternate s2, s1, ..; the tail reads the last one.  out: fp32 [B N,3,4H,4W], every element written once.  stages: which
 * layers run, each on the scratch as it stands.  Frame 0 of each clip takes warp = e_0 and flow = 0 and never reads the previous
 * clip.  Allocates nothing, never synchronises; -2 = invalid arguments (a NULL buffer, nb < 1, flows NULL with N > 1, stages outside
 * the mask), -1 = unsupported geometry (B N > 65535, H or W > 8192, nb > 1024, dtype), every buffer untouched. */
#define SR_MF_ENCODER 1
#define SR_MF_FIRST 2
#define SR_MF_BLOCKS 4
#define SR_MF_TAIL 8
#define SR_MF_ALL 15
int sr_mf_net_fwd(const float* frames, const float* flows, const void* blob, const void* head_blob, void* s0, void* s1, void* s2,
                  float* out, int nb, int B, int N, int H, int W, int dtype, int stages, sr_stream_t stream);

/* ---- multi-frame video network, the training route (csrc/multi_frame.h, csrc/multi_frame_bwd.h, csrc/result_block.h) ----
 * sr_mf_net_train_fwd is sr_mf_net_fwd (the same instructions per output, bit-identical out) that keeps what the backward reads, all
 * caller-owned, images [B N,H,W,32] in `dtype`: acts = nb + 1 images (acts[0] = e, acts[i] = block i's input = block i - 1's output,
 * acts[nb] = the tail's input); ts = nb images (block i's t = ReLU(conv1)); masks = nb x [B N,H,W] uint32 (bit c: conv1's fp32
 * accumulator of channel c > 0); wf = 2 images: wf[0] = block 0's warp operand as staged (frame 0 of a clip: a copy of e_0), wf[1] =
 * the flow rounded to `dtype` in channels 0, 1 and zeros in 2..31 (frame 0 of a clip: all zero).  stages: SR_MF_ENCODER .. SR_MF_TAIL.
 *
 * sr_mf_net_bwd: g: d(loss)/d(out), contiguous fp32 [B N,3,4H,4W]; flow_bound: DEVICE scalar >= max |flow| (sizes the warp
 * backward's window; flows and flow_bound may be NULL when N == 1); bwd_blob: packing.mf_bwd_tables layout in `dtype`; gs: six
 * [B N,H,W,32] scratch images: block i = nb - 1 .. 1 reads its dy from gs[0] / gs[1] (the tail writes gs[0]) and writes dx into the
 * other, block 0 writes de_direct there too; gs[2] = dt and, after SR_MF_BWD_WARP, de; gs[3] = dwarp; gs[4..5] = dD as [B N,H,W,48].
 * parts: fp32 workgroup slabs, (2 nb + 3) x wgs x 32768 + wgs x 3072 floats (packing.mf_bwd_parts); 1 <= wgs <= 1024.  grads (fp32, C
 * = the model's channels), packing.mf_grad_sizes' order: per block dW1 | db1 | dW2 | db2 (block 0's dW1 is (C, 2C + 2, 3, 3) over
 * cat(flow, warp, e)), decode dW (48,C,3,3) | db (48), encoder dW (C,3,3,3) | db (C); only the sections of the stages that ran are
 * written.  stages: which layers run, each on gs as it stands.  No atomics; no flow and no frame gradient.
 * Both: allocate nothing, never synchronise; -2 = invalid arguments, -1 = unsupported geometry (as sr_mf_net_fwd, or more than
 * 2^31 - 1 frames x 8 x 16 tiles), every buffer untouched.  Added without a change of sr_abi_version(). */
#define SR_MF_BWD_TAIL 1
#define SR_MF_BWD_BLOCKS 2
#define SR_MF_BWD_FIRST 4
#define SR_MF_BWD_WARP 8
#define SR_MF_BWD_ENCODER 16
#define SR_MF_BWD_ALL 31
int sr_mf_net_train_fwd(const float* frames, const float* flows, const void* blob, const void* head_blob, void* acts, void* ts,
                        unsigned* masks, void* wf, float* out, int nb, int B, int N, int H, int W, int dtype, int stages,
                        sr_stream_t stream);
int sr_mf_net_bwd(const float* frames, const float* flows, const float* flow_bound, const float* g, const void* bwd_blob,
                  const void* acts, const void* ts, const unsigned* masks, const void* wf, void* gs, float* parts, int wgs, float* grads,
                  int C, int nb, int B, int N, int H, int W, int dtype, int stages, sr_stream_t stream);
/* sr_mf_net_bwd with the trainers' loss folded into its first stage, as sr_fn_net_bwd_loss: in place of g, sr = the network's output
 * and hr = the target, both contiguous fp32 [B N,3,4H,4W]; the un-shuffled gradient image dD is formed from them (one launch walking
 * 8 x 32 LR tiles) instead of being read from g.  loss_part: min(B N x ceil(H / 8) x ceil(W / 32), wgs) floats, one per workgroup of
 * that stage.  stages must include SR_MF_BWD_TAIL.  Added without a change of sr_abi_version(). */
int sr_mf_net_bwd_loss(const float* frames, const float* flows, const float* flow_bound, const float* sr, const float* hr, int loss_kind,
                       float gscale, float* loss_part, const void* bwd_blob, const void* acts, const void* ts, const unsigned* masks,
                       const void* wf, void* gs, float* parts, int wgs, float* grads, int C, int nb, int B, int N, int H, int W,
                       int dtype, int stages, sr_stream_t stream);

/* ---- the video networks' one-call training step (csrc/clip_param_step.h around the four entry points above) ----
 * One call = weight norm of the weight-normed convs and gather of every trained tensor into `src` (one launch per SR_CLIP_STEP_CAP
 * tensors), the index packing of the three blobs (one launch), sr_*_net_train_fwd, sr_*_net_bwd_loss with gscale = 1 / numel, and the
 * weight-norm backward onto (weight_g, weight_v) with torch.optim.Adam's step of every trained tensor (one launch per
 * SR_CLIP_STEP_CAP tensors; sr_adam_step's arithmetic from the fp32 gradient times loss_weight).  No gradient tensor of a parameter
 * is written.
 * params: n_params rows in any order.  p1 != NULL: a weight-normed conv, p0 = weight_g (rows), p1 = weight_v (rows x len, the norm runs
 * over len), (m0, v0) / (m1, v1) = exp_avg / exp_avg_sq of p0 / p1.  p1 == NULL: a plain tensor p0 of len elements with (m0, v0); rows
 * is ignored.  src_off: where the effective tensor goes in src (packing.fn_tables / mf_tables' canonical source; the caller keeps the
 * constants the indices read, src itself is scratch); grad_off: the tensor's place in `grads` (sr_fn_net_bwd's / sr_mf_net_bwd's
 * order).  inv: scratch, one float per weight-normed row (1 / |v|).  idx[j] (DEVICE, n_idx[j] int64 offsets into src, each < src_n:
 * not checked) -> blob[j] in `dtype`, 16-byte aligned: j = 0 the forward blob, 1 the backward blob, 2 the encoder's head blob.
 * adam: sr_adam_step's scalars of this step.  *loss_out (device) = loss_weight x the mean loss.  The remaining arguments are those of
 * the entry points above; `out` receives the network's output, loss_part the per-workgroup loss sums (wgs floats suffice).
 * Allocates nothing, never synchronises; -2 = invalid arguments, -1 = unsupported geometry / dtype, nothing launched in either case.
 * Added without a change of sr_abi_version(). */
#define SR_CLIP_STEP_CAP 48
typedef struct {
  float* p0; float* p1; float* m0; float* v0; float* m1; float* v1;
  long src_off, grad_off;
  int rows, len;
} sr_clip_param_t;
typedef struct {
  const sr_clip_param_t* params; int n_params;
  float* src; long src_n;
  float* inv; long inv_n;
  const long* idx[3]; void* blob[3]; long n_idx[3];
  const sr_adam_t* adam; float loss_weight; float* loss_out;
} sr_clip_step_t;
int sr_fn_net_train_step(const sr_clip_step_t* step, const float* frames, const float* hr, int loss_kind, const long* conv_off,
                         void* acts, void* ts, unsigned* masks, float* out, void* gs, float* parts, int wgs, float* grads,
                         float* loss_part, int C, int nb, int N, int H, int W, int dtype, sr_stream_t stream);
/* sr_fn_net_train_step at any output size: out and hr are fp32 [N,3,OH,OW], the forward is sr_fn_net_train_fwd_sized and the backward
 * sr_fn_net_bwd_loss_sized with gscale = 1 / (N 3 OH OW) (an fp32 quotient) over the tables of sr_fn_net_fwd_sized; the weight norm
 * is formed in torch._weight_norm's arithmetic (clip_wn_fwd_aten_kernel), so `out` equals sr_fn_net_fwd_sized on blobs packed from
 * torch's effective weights bit for bit; the other parameter stages are unchanged.  -2 also for a NULL table or OH, OW < 1, -1 also
 * beyond SR_FN_MAX_OUT, nothing launched in either case.  Added without a change of sr_abi_version(). */
int sr_fn_net_train_step_sized(const sr_clip_step_t* step, const float* frames, const float* hr, int loss_kind, const long* conv_off,
                               void* acts, void* ts, unsigned* masks, float* out, int OH, int OW, const int* ty, const float* ly,
                               const int* tx, const float* lx, void* gs, float* parts, int wgs, float* grads, float* loss_part, int C,
                               int nb, int N, int H, int W, int dtype, sr_stream_t stream);
int sr_mf_net_train_step(const sr_clip_step_t* step, const float* frames, const float* flows, const float* flow_bound, const float* hr,
                         int loss_kind, void* acts, void* ts, unsigned* masks, void* wf, float* out, void* gs, float* parts, int wgs,
                         float* grads, float* loss_part, int C, int nb, int B, int N, int H, int W, int dtype, sr_stream_t stream);

/* ---- hardware probes used by tests/test_gpu_probe.py (lane maps the kernels rely on) ---- */
int sr_probe_mfma_bf16(const void* a_frag, const void* b_frag, float* acc_out, sr_stream_t stream);
int sr_probe_mfma_f32(const float* a_frag, const float* b_frag, float* acc_out, sr_stream_t stream);
int sr_probe_tr_read(const void* img_bf16, int n_elems, const int* lane_elem_off, void* out_bf16x4,
                     sr_stream_t stream);
/* streaming copy of n_bytes (multiple of 16): the achievable-HBM-bandwidth yardstick for bench.py */
int sr_probe_copy(const void* src, void* dst, size_t n_bytes, sr_stream_t stream);
/* Launch-floor probe: `reps` dependent launches of an empty kernel with the given grid, workgroup size and
 * dynamic LDS; writes gx*gy words to `out`.  Timing it gives the fixed cost under every chained kernel. */
int sr_probe_launch_floor(void* out, int gx, int gy, int threads, int lds_bytes, int reps, sr_stream_t stream);
/* The same chain captured in a hipGraph and replayed `iters` times (synchronous; result in *us_per_launch). */
int sr_probe_launch_floor_graph(void* out, int gx, int gy, int threads, int lds_bytes, int reps, int iters,
                                float* us_per_launch, float* host_us_per_graph /* may be NULL */);
/* Debug: in the diagnostic build (libsr_hotpath_dbg.so, `python -m mobilesuperresolution_amd.build --debug`) the
 * instrumented kernels write s_memrealtime stamps to buf[n_workgroups][16 waves][16 stamps][2] u64 (NULL = off); workgroups
 * beyond n_workgroups do not stamp.  The product library contains no stamp code and returns -1. */
int sr_debug_set_stamps(void* buf, long n_workgroups);

#ifdef __cplusplus
}
#endif
#endif /* SR_HOTPATH_H */
