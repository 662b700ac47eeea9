/* libcontrad_hip.so -- C ABI of the MI355X-native (gfx950) ContraD discriminator-step hot path.
 *
 * Drop-in boundary B2 of SURVEY.md section 8(b): the reference's only native interface is two
 * pybind11 torch extensions JIT-built at import (models/gan/stylegan2/op/upfirdn2d.cpp:12-23,
 * op/fused_bias_act.cpp:11-21); everything else on the path reaches cuDNN/ATen through PyTorch
 * (F.conv2d, F.linear, grid_sample, spectral_norm, log_softmax, optim.Adam).  This library replaces
 * all of them with hand-written HIP kernels behind one convention:
 *
 *   - plain C: raw DEVICE pointers (fp32 unless noted) + sizes; no torch types, no hidden allocation,
 *     no host synchronisation, re-entrant; every launcher enqueues on the caller's `stream`
 *     (a hipStream_t passed as void*);
 *   - outputs and workspaces are caller-allocated;
 *   - a workspace holds exactly what its `contrad_*_workspace_bytes` query answers (more is allowed), 16-byte aligned; its
 *     contents on entry are undefined and mean nothing after the call returns, and nothing outside
 *     [workspace, workspace + workspace_bytes) is written (tests/test_workspace_contract_gpu.py);
 *   - return value 0 = ok, >0 = hipError_t of the launch, <0 = -EINVAL style argument error
 *     (the Python host raises RuntimeError, mirroring TORCH_CHECK in the reference's .cpp shims).
 *
 * Internal activation layout is NHWC ("pixel-major": a pixel's channels are contiguous, `ld*` floats
 * between pixels); the Python module boundary stays NCHW like the reference.  Weights are consumed in
 * a packed GEMM layout Wp[(kh*KW+kw)*Cin + c][Cout] produced by contrad_weight_prep_* below.
 */
#ifndef CONTRAD_HIP_H
#define CONTRAD_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void* contrad_stream_t; /* hipStream_t */

int contrad_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * Convolution / linear engine: implicit-GEMM on v_mfma_f32_32x32x2_f32, fp32 in / fp32 accumulate.
 * Replaces F.conv2d fwd + dgrad + wgrad (models/gan/sndcgan.py:91-109, stylegan2/layers.py:115-121),
 * nn.ConvTranspose2d forward (= dgrad; sndcgan.py:26-38) and F.linear (conv with H=W=KH=KW=1;
 * models/gan/base.py:14-35,92-101).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int N, H, W, C;   /* input  tensor: batch, height, width, channels (Cin)            */
  int ldx;          /* floats between consecutive input pixels  (>= C, multiple of 4)  */
  int Ho, Wo, K;    /* output tensor: height, width, channels (Cout)                   */
  int ldy;          /* floats between consecutive output pixels (>= K)                 */
  int KH, KW;       /* filter size                                                     */
  int stride, pad;  /* same in both dims; stride in {1,2}                              */
  int ldw;          /* floats between rows of the packed weight [KH*KW*C][ldw] (>= K)  */
} contrad_conv_desc;

/* Sizes: N * H * W * ldx, N * Ho * Wo * ldy and KH * KW * C * ldw are each below 2^31 ELEMENTS (leading dimensions counted):
 * every entry point returns -EINVAL and every plan / workspace / *_ok query -22 from 2^31 on.  Bytes are not limited: an
 * operand may span up to 8 GiB, base pointers are 64-bit.  What is relative to a block's or an image's base is a 32-bit byte
 * offset below 2^31: a shape whose block would reach further (nimg * H * W * max(ldi, ldo) * 4 >= 2^31 for a Winograd family,
 * one image of 2^31 bytes for the branch-free FIR forms of contrad_upfirdn2d) is refused by that family's guard and runs on a
 * family that can address it -- slower, never wrong (tests/test_far_offsets_gpu.py, tests/test_far_offsets_cpu.py).
 *
 * Alignment: when the channel counts / leading dimensions are multiples of 4 the kernels use 16-byte accesses, and
 * x, wp, y, gy, dx, act_ref and the workspaces must then be 16-byte aligned (-EINVAL otherwise).
 *
 * y[n,ho,wo,k] = gain * lrelu_slope( sum_{kh,kw,c} x[n,ho*s-p+kh,wo*s-p+kw,c] * wp[(kh,kw,c),k] + bias[k] )
 * bias may be NULL; slope = 1 disables the activation. */
int contrad_conv2d_fwd(const contrad_conv_desc* d, const float* x, const float* wp, const float* bias,
                       float* y, float slope, float gain, float* workspace, long long workspace_bytes,
                       contrad_stream_t stream);
/* Same with a residual addend: y = gain * lrelu_slope(conv + bias) + addend, `addend` (may be NULL) a tensor of y's
 * shape and leading dimension (may alias nothing).  The ResBlock merge (out + skip) of the StyleGAN2 discriminator
 * (models/gan/stylegan2/discriminator.py:72-74) is the epilogue of its 1x1 skip convolution this way. */
int contrad_conv2d_fwd_add(const contrad_conv_desc* d, const float* x, const float* wp, const float* bias,
                           const float* addend, float* y, float slope, float gain, float* workspace,
                           long long workspace_bytes, contrad_stream_t stream);
/* Scratch for the split-K partial slabs of small-M / deep-K shapes (the merged head GEMM); 0 for most shapes, in
 * which case workspace may be NULL. */
long long contrad_conv2d_fwd_workspace_bytes(const contrad_conv_desc* d);

/* dx[n,h,w,c] = act'(act_ref[n,h,w,c]) * sum_{kh,kw,k} gy[n,(h+p-kh)/s,(w+p-kw)/s,k] * wp[(kh,kw,c),k]
 * act_ref (may be NULL) is the OUTPUT of the leaky-relu that produced this conv's input (same layout
 * as dx, leading dimension ldx): act' = gain * (act_ref > 0 ? 1 : slope).
 * Stride-2 is decomposed into s*s output-parity classes so only contributing taps are multiplied. */
int contrad_conv2d_dgrad(const contrad_conv_desc* d, const float* gy, const float* wp, float* dx,
                         const float* act_ref, float slope, float gain, contrad_stream_t stream);
/* Same, with a scratch buffer: small-M / deep-K stride-1 layers (the 4x4 and 8x8 levels at small per-rank batches) then
 * split the contraction into deterministic partial slabs (dx's layout) that a second kernel sums in fixed order before
 * the fused act' epilogue.  workspace may be NULL (never splits); size from contrad_conv2d_dgrad_workspace_bytes. */
long long contrad_conv2d_dgrad_workspace_bytes(const contrad_conv_desc* d);
int contrad_conv2d_dgrad_ws(const contrad_conv_desc* d, const float* gy, const float* wp, float* dx,
                            const float* act_ref, float slope, float gain, float* workspace,
                            long long workspace_bytes, contrad_stream_t stream);

/* Supported shapes of the 3x3 stride-1 pad-1 Winograd kernels (contrad_conv2d_wino_ok / contrad_conv2d_wino44_ok; the same
 * statement stands in ops.conv2d_wino and csrc/wino44.h):
 *   F(2x2, 3x3): H and W powers of two >= 4, any aspect ratio; input channels a multiple of 16, output channels of 64;
 *   F(4x4, 3x3): H and W powers of two, either square 4x4 / 8x8 / 16x16, or W >= 32 and H >= 16; input and output channels
 *                multiples of 32;
 *   both: input and filter leading dimensions multiples of 4, block-relative offsets below 2^31 bytes.  "Input" / "output" are
 *   those of the call: x / y in mode 0, gy / dx in mode 1.  contrad_conv2d_wino_workspace_bytes (every mode) and
 *   contrad_conv2d_wino44_workspace_bytes (when neither mode is accepted) return -22 exactly where the *_ok query says 0.
 *
 * Winograd F(2x2, 3x3) in exact fp32 (csrc/wino.h) for 3x3 stride-1 pad-1 layers on the maps above: 2.25x fewer multiply-adds than the direct kernels,
 * fp32 round-off class results (rel-L2 3 - 6e-7 against fp64; F.conv2d of the reference reaches cuDNN's Winograd-class
 * kernels the same way: models/gan/sndcgan.py:91-109, models/gan/stylegan2/layers.py:115-121).  contrad_conv2d_fwd_add /
 * contrad_conv2d_dgrad_ws choose it by themselves for launches of about one item (64 tiles x 64 output channels) per CU or
 * more -- their *_workspace_bytes then cover the transformed filter (16 * C * K floats, rewritten by every call) --;
 * contrad_conv2d_wino runs it on ANY shape contrad_conv2d_wino_ok accepts (parity tests, integrators with their own plan).
 * mode 0: in = x, out = y = gain * lrelu(conv + bias) [+ ref], bias / ref may be NULL;
 * mode 1: in = gy, out = dx [* act'(ref)], bias must be NULL (semantics of contrad_conv2d_fwd_add / _dgrad_ws).
 * The weight gradient of the same layers (mode 2: F(3x3, 2x2), input AND output channels multiples of 64) runs on
 * wino_wgrad_kernel: contrad_conv2d_wgrad picks it when every CU gets a long enough share of the tiles,
 * contrad_conv2d_wino_wgrad forces it (arguments and results of contrad_conv2d_wgrad, workspace = split slabs).
 * The same entry points serve the strided layers: 4x4 stride 2 pad 1 (csrc/wino22.h, all three modes) and, mode 0 only, 3x3
 * stride 2 pad 0 on a (2G + 1) x (2G + 1) map (csrc/wino23.h: StyleGAN2's blurred down-sampling convolution, models/gan/
 * stylegan2/layers.py:174-198; F(2x2, 2x2) on the four input phases with the structurally zero planes skipped: 25 / 36 of the
 * dense layer's multiply-adds; contrad_conv2d_path = 10). */
int contrad_conv2d_wino_ok(const contrad_conv_desc* d, int mode);
long long contrad_conv2d_wino_workspace_bytes(const contrad_conv_desc* d, int mode);
int contrad_conv2d_wino_wgrad(const contrad_conv_desc* d, const float* x, const float* gy, float* dwp, float* dbias,
                              float* workspace, long long workspace_bytes, contrad_stream_t stream);
int contrad_conv2d_wino(const contrad_conv_desc* d, int mode, const float* in, const float* wp, const float* bias,
                        const float* ref, float* out, float slope, float gain, float* workspace,
                        long long workspace_bytes, contrad_stream_t stream);

/* Winograd F(4x4, 3x3) in fp32 (csrc/wino44.h) for the same 3x3 stride-1 pad-1 layers on the maps stated above (output
 * channels in whole 64-wide blocks: wino44_kernel; an odd number of 32-wide blocks -- StyleGAN2_512's 32 -> 32 channel
 * layers -- and the 4x4 maps: csrc/wino44n.h): 2.25 multiply-adds per output instead of 4
 * (F(2x2, 3x3)) or 9 (direct); standard interpolation points (0, +-1, +-2, inf), round-off rel-L2 1 - 5e-6 against fp64 (the
 * contract of this path is 1e-3; reference as above: F.conv2d of models/gan/sndcgan.py:91-109, stylegan2/layers.py:115-121).
 * contrad_conv2d_fwd_add / contrad_conv2d_dgrad_ws choose it ahead of F(2x2, 3x3) for launches of a full round of its items
 * (512 output pixels x 64 or 32 output channels per CU) -- their *_workspace_bytes then cover 36 * C * K floats --;
 * contrad_conv2d_wino44 forces it on any shape contrad_conv2d_wino44_ok accepts (arguments and semantics of
 * contrad_conv2d_wino, modes 0 and 1). */
int contrad_conv2d_wino44_ok(const contrad_conv_desc* d, int mode);
long long contrad_conv2d_wino44_workspace_bytes(const contrad_conv_desc* d);
int contrad_conv2d_wino44(const contrad_conv_desc* d, int mode, const float* in, const float* wp, const float* bias,
                          const float* ref, float* out, float slope, float gain, float* workspace,
                          long long workspace_bytes, contrad_stream_t stream);

/* Transformed Winograd filters made ahead of the convolutions (csrc/igemm.hip: filter_prep_kernel).  The entry points above
 * rebuild U = G g G^T from the packed weight in a small launch of their own on every call; a network whose packed weights
 * all come from one contrad_sn_weight_prep makes every U it needs in ONE launch right after it and hands each to the
 * call that consumes it:
 *   1. contrad_conv2d_filter_kind(d, mode, &bytes): which transformed filter contrad_conv2d_fwd_add (mode 0) /
 *      contrad_conv2d_dgrad_ws (mode 1) read for this descriptor WHEN GIVEN THEIR WORKSPACE -- 0: none (a direct kernel),
 *      else the contrad_conv2d_path number of the family: 7 F(2x2,3x3), 8 F(2x2,2x2) on 4x4 stride 2, 9 F(4x4,3x3) (paths
 *      9 and 11 read the same U), 10 F(2x2,2x2) on 3x3 stride 2 -- and its size in bytes (16 / 36 / 36 / 36 * C * K
 *      floats; *bytes = 0 for kind 0; bytes may be NULL).  The plan depends on the whole descriptor, N included.
 *      Negative = bad descriptor.
 *   2. contrad_conv2d_filter_prep(batch): fills every job's U (caller-allocated, 16-byte aligned, `bytes` long) from
 *      its packed weight wp [KH*KW*C][ldw]; C, K, ldw are the descriptor's.  One launch for the whole batch; U's bits
 *      are those the per-call transform writes.  -22 for an unknown kind / mode, misaligned pointers or n out of range.
 *   3. contrad_conv2d_fwd_add_u / contrad_conv2d_dgrad_ws_u: contrad_conv2d_fwd_add / contrad_conv2d_dgrad_ws with the
 *      job `u` (a HOST struct, read during the call only; may be NULL) whose U was prepared.  The call checks on the host
 *      that `u` fits the path it is about to take -- same kind as the plan of (d, mode) with this workspace, same mode, C, K,
 *      ldw and the same wp pointer -- and then launches the main kernel alone, reading u->U; otherwise it behaves exactly
 *      like the entry point without `_u` (per-call transform into `workspace`, or a direct kernel).  The workspace
 *      arguments keep their meaning: a call without the workspace of *_workspace_bytes does not take a Winograd path,
 *      with or without `u`.  The caller keeps u->U unchanged from the prep until the consuming launch has run. */
#define CONTRAD_FILTER_MAX_JOBS 16
typedef struct {
  const float* wp;   /* packed weight [KH*KW*C][ldw]                                              */
  float* U;          /* transformed filter (out of the prep, in of the conv call)                 */
  int kind;          /* 7, 8, 9 or 10: contrad_conv2d_filter_kind                                 */
  int mode;          /* 0: for contrad_conv2d_fwd_add_u, 1: for contrad_conv2d_dgrad_ws_u         */
  int C, K, ldw;     /* the descriptor's input channels, output channels, packed leading dimension */
} contrad_filter_job;
typedef struct {
  int n;
  contrad_filter_job jobs[CONTRAD_FILTER_MAX_JOBS];
  int block_start[CONTRAD_FILTER_MAX_JOBS + 1]; /* filled by the launcher */
} contrad_filter_batch;
int contrad_conv2d_filter_kind(const contrad_conv_desc* d, int mode, long long* bytes);
int contrad_conv2d_filter_prep(const contrad_filter_batch* b, contrad_stream_t stream);
int contrad_conv2d_fwd_add_u(const contrad_conv_desc* d, const float* x, const float* wp, const float* bias,
                             const float* addend, float* y, float slope, float gain, float* workspace,
                             long long workspace_bytes, const contrad_filter_job* u, contrad_stream_t stream);
int contrad_conv2d_dgrad_ws_u(const contrad_conv_desc* d, const float* gy, const float* wp, float* dx,
                              const float* act_ref, float slope, float gain, float* workspace,
                              long long workspace_bytes, const contrad_filter_job* u, contrad_stream_t stream);

/* dwp[(kh,kw,c),k] = sum_{n,ho,wo} x[n,ho*s-p+kh,wo*s-p+kw,c] * gy[n,ho,wo,k]      (split over the
 * n*ho*wo axis into deterministic partial slabs in `workspace`, then reduced in fixed order).
 * dbias (may be NULL; needs C, K, ldx, ldy multiples of 4): dbias[k] = sum_{n,ho,wo} gy[n,ho,wo,k], the bias
 * gradient, accumulated for free from the gy tiles the kernel streams anyway. */
long long contrad_conv2d_wgrad_workspace_bytes(const contrad_conv_desc* d);
/* Introspection for profiling: block tile (bm x bn x 32) the launcher picks for `mode` (0 fwd, 1 dgrad,
 * 2 wgrad) on this geometry, i.e. which igemm_kernel<mode, bm, bn> instance runs when the layer is the igemm engine's
 * (contrad_conv2d_path 0 - 3; for the other families: the tile it would take). */
int contrad_conv2d_tile(const contrad_conv_desc* d, int mode, int* bm, int* bn);
/* Which kernel family serves this shape: 0 = general scalar-gather (igemm_kernel<..., false>), 1 = general float4
 * (igemm_kernel<..., true>), 2 = lean loop (igemm_lean_kernel), 3 = lean loop on tiles that skip padding taps (small maps:
 * pixel-major tiles -- the rows of a tile are images at one output pixel -- or border classes -- (image, pixel) rows inside
 * a rectangle of pixels that share their non-padding taps), 4 = the accumulator-stationary weight-gradient kernel of
 * the 32 -> 32 channel 3x3 layers (wgrad_c32_kernel, mode 2 only), 5 = the single-output 1x1 layer (fwd_k1_kernel, mode 0
 * only: the 512 -> 1 logit of the heads), 6 = the weight-stationary kernel of the 32 -> 32 channel 3x3 stride-1 layers
 * (conv_c32_kernel<mode>, modes 0 and 1), 7 = Winograd F(2x2, 3x3) (wino_kernel<mode>, modes 0 and 1; with a workspace) / F(3x3, 2x2) (wino_wgrad_kernel, mode 2),
 * 8 = F(2x2, 2x2) on the phases of the 4x4 stride-2 layers (wino22_kernel<mode> / wino22_wgrad_kernel), 9 = Winograd F(4x4, 3x3)
 * (wino44_kernel<mode>, modes 0 and 1; with a workspace), 10 = F(2x2, 2x2) on the phases of a 3x3 stride-2 pad-0 layer with the zero
 * planes skipped (wino23_kernel, mode 0; with a workspace), 11 = F(4x4, 3x3) with 32-wide output-channel blocks (wino44n_kernel<mode>:
 * output channels not a multiple of 64, and the 4x4 maps; with a workspace);  negative = bad descriptor.  Profiling aid.
 * Workspace assumption: this and contrad_conv2d_executed_fraction describe the plan of a call that passes a workspace of
 * contrad_conv2d_{fwd,dgrad,wgrad}_workspace_bytes.  contrad_conv2d_fwd_add / contrad_conv2d_dgrad_ws with a NULL (or
 * smaller) workspace skip paths 7 - 11 and run the direct kernels instead (contrad_conv2d_dgrad: never split-K either).
 * The launchers and every plan query here (path, filter_kind, *_workspace_bytes, executed_fraction, grid_blocks,
 * tile_order) read ONE route decision (csrc/igemm.hip: conv_route), so what they report is what a launch does. */
int contrad_conv2d_path(const contrad_conv_desc* d, int mode);
/* Share of the layer's nominal multiply-adds (2*N*Ho*Wo*K*C*KH*KW, the count every roofline here is quoted on, padding
 * taps included as in the reference's dense layer) that the kernel actually issues: 1 except on pixel-major tiles (path
 * 3), which skip the tap-positions that read padding (0.69 for a 3x3 pad-1 layer on a 4x4 map), and on the Winograd path
 * (7): 4/9, (8): 9/16, (9) and (11): 1/4, (10): 25/36 -- the transform-domain multiply-adds.  (A weight-gradient tile
 * that also sums the bias gradient visits everything: not reflected.)  Profiling aid. */
double contrad_conv2d_executed_fraction(const contrad_conv_desc* d, int mode);
/* Workgroups (256 threads each) of the main igemm launch this geometry gets for `mode` (with_workspace != 0: the plan the
 * *_ws entry points use, i.e. split-K allowed).  Profiling aid: lets a rocprofv3 kernel trace, which names only the
 * template instance, be joined to the layer shape a dispatch served (tools/rocpd_rows.py); negative = bad descriptor. */
long long contrad_conv2d_grid_blocks(const contrad_conv_desc* d, int mode, int with_workspace);
/* Pixel-major launches (path 3, mode 0 / 1) with at most 256 M-tiles per table: the order in which the launch walks its
 * M-tiles, out[i] = image block * pixels + pixel of the i-th M-tile (for the strided data gradient: of every parity class,
 * the pixel mirrored along the class's odd axes), chosen so that the tiles a CU is dealt -- an XCD's blocks go round-robin
 * over its 32 CUs -- carry equal work.  Returns the number of entries written, 0 when the launch uses no such table
 * (image-major tiles, border classes, more than 256 tiles), negative = bad argument.  For a layer the plan gives to
 * Winograd (path 7 - 11) this is the table of the direct route a call without the filter workspace falls through to.
 * Host logic only; lets the plan be
 * tested without a GPU (tests/test_abi_cpu.py). */
int contrad_conv2d_tile_order(const contrad_conv_desc* d, int mode, unsigned char* out, int capacity);
int contrad_conv2d_wgrad(const contrad_conv_desc* d, const float* x, const float* gy, float* dwp,
                         float* dbias, float* workspace, long long workspace_bytes, contrad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Contrastive losses: fused pairwise-cosine + log-sum-exp, S = Z Z^T / temp never written to HBM.
 * Replaces nt_xent (training/criterion.py:24-45; mode 0, R = 2N) and supcon_fake
 * (training/gan/contrad.py:8-32; mode 1, R = 3N, anchors = rows 2N..3N) incl. their autograd backward,
 * and F.normalize (contrad.py:43,48).
 * ---------------------------------------------------------------------------------------------- */
/* Scratch for the column-split partials of either call (the R x R work is spread over ~256 blocks; the
 * per-split (max, sum, target) triples / dZ slabs are merged in a fixed order -> deterministic). */
long long contrad_contrast_workspace_bytes(int R, int D);
/* z[R,D] row-normalised, D <= 256. Writes lse[R], rowloss[R] (scratch) and loss[0] = mean anchor loss.
 * Mode 1 needs N >= 2 (with one fake an anchor has no positive); both calls return -22 otherwise. */
int contrad_contrast_fwd(const float* z, int R, int D, int N, int mode, float inv_temp, float* lse,
                         float* rowloss, float* loss, float* workspace, long long workspace_bytes,
                         contrad_stream_t stream);
/* dz[R,D] = (grad_scale ? grad_scale[0] : 1) * d loss / d z   (lse from contrad_contrast_fwd). */
int contrad_contrast_bwd(const float* z, const float* lse, int R, int D, int N, int mode, float inv_temp,
                         const float* grad_scale, float* dz, float* workspace, long long workspace_bytes,
                         contrad_stream_t stream);
/* z = u / max(||u||_2, eps) per row; inv_norm[R] kept for the backward. */
int contrad_l2norm_fwd(const float* u, int ldu, float* z, float* inv_norm, int R, int D, float eps,
                       contrad_stream_t stream);
/* du (+)= (dz - z <z,dz>) * inv_norm */
int contrad_l2norm_bwd(const float* dz, const float* z, const float* inv_norm, float* du, int ldu, int R,
                       int D, int accumulate, contrad_stream_t stream);

/* The same four calls on up to two independent problems per launch (ContraD's D-step runs NT-Xent on 2N rows and SupCon
 * on 3N rows; each alone fills a fraction of the chip): one grid over both for the main kernel and one for each reduce.
 * Every problem keeps its own column splits, workspace (contrad_contrast_workspace_bytes each, disjoint) and fixed summation
 * order, so each result is bitwise that of the single-problem call.  Problems whose D fall into different kernel instances
 * (D <= 64, <= 128, <= 256) are launched one after the other.  `p` is a HOST array, read during the call only.
 *   forward:  reads z, R, D, N, mode, inv_temp;  writes lse[R], rowloss[R], loss[1].
 *   backward: reads z, lse, grad_scale (may be NULL);  writes dz[R,D]. */
#define CONTRAD_CONTRAST_MAX_PROBLEMS 2
typedef struct {
  const float* z;          /* [R][D] row-normalised                                   */
  int R, D, N, mode;
  float inv_temp;
  float* lse;              /* [R]  out of the forward, in of the backward             */
  float* rowloss;          /* [R]  forward scratch                                    */
  float* loss;             /* [1]  forward out                                        */
  const float* grad_scale; /* backward, may be NULL                                   */
  float* dz;               /* [R][D] backward out                                     */
  float* workspace;
  long long workspace_bytes;
} contrad_contrast_problem;
int contrad_contrast_fwd_batched(const contrad_contrast_problem* p, int n, contrad_stream_t stream);
int contrad_contrast_bwd_batched(const contrad_contrast_problem* p, int n, contrad_stream_t stream);
/* contrad_l2norm_fwd / _bwd on up to two matrices per launch.  Backward only: rows [R, R + zero_rows) of du are set to
 * zero by the same launch (the projection rows a loss does not read get their zero gradient without a fill of their own). */
typedef struct {
  const float* u;          /* forward in  [R][ldu]                                    */
  float* z;                /* [R][D]  forward out, backward in                        */
  float* inv_norm;         /* [R]     forward out, backward in                        */
  const float* dz;         /* [R][D]  backward in                                     */
  float* du;               /* [R + zero_rows][ldu] backward out                       */
  int ldu, R, D;
  int accumulate;          /* backward: du += (rows below R only)                     */
  int zero_rows;
} contrad_l2norm_problem;
int contrad_l2norm_fwd_batched(const contrad_l2norm_problem* p, int n, float eps, contrad_stream_t stream);
int contrad_l2norm_bwd_batched(const contrad_l2norm_problem* p, int n, contrad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Weight preparation, batched over the layers of a network: spectral normalisation (one power
 * iteration per forward in training mode, u/v updated in place -- torch.nn.utils.spectral_norm as
 * applied at models/gan/sndcgan.py:111-118) or a fixed runtime scale (EqualConv2d/EqualLinear,
 * models/gan/stylegan2/layers.py:104,117,141), fused with the OIHW -> packed-GEMM-layout transpose.
 * ---------------------------------------------------------------------------------------------- */
#define CONTRAD_SN_MAX_LAYERS 24
#define CONTRAD_SN_MAX_PARTIALS 256
typedef struct {
  const float* w;    /* [K][C*T] original weight (OIHW flattened; column = c*T + tap)            */
  float* u;          /* [K]   left singular vector estimate (in/out)      (NULL if fixed_scale)  */
  float* v;          /* [C*T] right singular vector estimate (in/out)     (NULL if fixed_scale)  */
  float* u_snap;     /* [K]   copy of the u used by THIS call (fwd: written; bwd: read); may be NULL  */
  float* v_snap;     /* [C*T] copy of the v used by THIS call (fwd: written; bwd: read); may be NULL  */
  float* wp;         /* [T*C][ldw] packed effective weight (out fwd, in bwd)                      */
  const float* gwp;  /* [T*C][ldw] gradient wrt wp            (backward only)                     */
  float* gw;         /* [K][C*T]   gradient wrt w (out)       (backward only)                     */
  int K, C, T, ldw;  /* T = KH*KW                                                                 */
  float fixed_scale; /* > 0: wp = w * fixed_scale, no spectral norm                               */
} contrad_sn_layer;
typedef struct {
  int n;
  contrad_sn_layer layers[CONTRAD_SN_MAX_LAYERS];
  long long scratch_off[CONTRAD_SN_MAX_LAYERS]; /* float offset of layer l's scratch, each at least
                                                   contrad_sn_scratch_floats(K, C, T) long            */
} contrad_sn_batch;

long long contrad_sn_scratch_floats(int K, int C, int T);
/* sigma_out[n]: per-layer sigma (1/fixed_scale for fixed layers), needed by the backward. */
int contrad_sn_weight_prep(const contrad_sn_batch* b, int training, float eps, float* scratch,
                           float* sigma_out, contrad_stream_t stream);
/* gw = (gwp - <gwp, wp> u v^T) / sigma, with the sigma, wp and u/v (u_snap/v_snap when given, else u/v)
 * of the matching forward. */
int contrad_sn_weight_grad(const contrad_sn_batch* b, float* scratch, const float* sigma,
                           contrad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * RGB ends of the networks (one GEMM dimension is 3 -> direct VALU kernels, HBM-bound).
 * ---------------------------------------------------------------------------------------------- */
/* First conv of D on the NCHW image with the x*2-1 input rescale fused (D_SNDCGAN.penultimate +
 * main.0, models/gan/sndcgan.py:91,123; StyleGAN2 FromRGB, stylegan2/discriminator.py:17-19,226):
 * y[n,h,w,:] = gain*lrelu_slope(conv_kxk(img*in_scale+in_shift) + bias), NHWC out; k in {1,3}, Cin = 3. */
int contrad_rgb_conv_fwd(const float* img, const float* wp, const float* bias, float* y, int N, int Cin,
                         int H, int W, int K, int k, int ldy, int ldw, float in_scale, float in_shift,
                         float slope, float gain, contrad_stream_t stream);
long long contrad_rgb_conv_wgrad_workspace_bytes(int N, int Cin, int H, int W, int K, int k);
/* dwp[(tap*Cin+ci)][k] and dbias[k] (may be NULL) from gy = gradient wrt the pre-activation output. */
int contrad_rgb_conv_wgrad(const float* img, const float* gy, float* dwp, float* dbias, int N, int Cin,
                           int H, int W, int K, int k, int ldy, int ldw, float in_scale, float in_shift,
                           float* workspace, long long workspace_bytes, contrad_stream_t stream);
/* The three RGB-end entry points index with 64-bit element offsets and have no element limit: gy of contrad_rgb_conv_dgrad may
 * hold more than 2^31 floats (tests/test_far_offsets_gpu.py runs 1030 x 512 x 512 x 16 into 4 GiB of images).
 * Stride-1 transposed conv onto C <= 4 channels, NHWC in -> NCHW out,
 * out = f(acc + bias + residual) * out_scale + out_shift, f = identity (act 0) or tanh (act 1); `mod` (may be
 * NULL) is a per-sample [N][K] modulation of the input channels, `residual` (may be NULL) an NCHW tensor:
 * G_SNDCGAN's last ConvTranspose2d+Tanh+0.5x+0.5 (models/gan/sndcgan.py:37-38,47), d loss / d image of D's first
 * conv, and StyleGAN2's ToRGB = 1x1 modulated conv + bias + upsampled skip (stylegan2/generator.py:122-143). */
int contrad_rgb_conv_dgrad(const float* gy, const float* wp, const float* bias, const float* mod,
                           const float* residual, float* out, int N, int C, int H, int W, int K, int k,
                           int ldy, int ldw, int act, float out_scale, float out_shift,
                           contrad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * HBM-bound helpers: column statistics, BatchNorm (generator forward), GAN logit losses, Adam.
 * ---------------------------------------------------------------------------------------------- */
/* out[0][c] = sum_r x[r][c] (and out[1][c] = sum_r x[r][c]^2 if with_sq) over M rows; bias gradients
 * (autograd of the "+ bias" in nn.Conv2d / nn.Linear) and BatchNorm batch statistics. */
long long contrad_colstats_workspace_bytes(long long M, int K, int with_sq);
int contrad_colstats(const float* x, long long M, int K, int ld, int with_sq, float* out, int accumulate,
                     float* workspace, long long workspace_bytes, contrad_stream_t stream);
/* nn.BatchNorm2d (train mode) + ReLU of G_SNDCGAN (models/gan/sndcgan.py:25-35,43): stats = {sum, sumsq}
 * over `count` rows (all ranks for SyncBatchNorm); perm_hw > 1 additionally maps column c*perm_hw+hw to
 * NHWC (hw, c) (the view(-1, 512, 4, 4) after norm_init, sndcgan.py:44). */
int contrad_bn_relu_apply(const float* x, float* y, long long M, int K, int ldx, int ldy, const float* stats,
                          float count, const float* gamma, const float* beta, float eps, int perm_hw,
                          contrad_stream_t stream);
/* The same in eval mode (G_SNDCGAN sampling from a checkpoint, cDDLS): mean[K] (running_mean minus the bias of the
 * producing layer when that layer ran without it) and var[K] (running_var) are used as they are, by the same kernel:
 * y = relu((x - mean) * rsqrt(var + eps) * gamma + beta).  -EINVAL on bad arguments before any GPU call. */
int contrad_bn_relu_apply_eval(const float* x, float* y, long long M, int K, int ldx, int ldy, const float* mean,
                               const float* var, const float* gamma, const float* beta, float eps, int perm_hw,
                               contrad_stream_t stream);
/* Backward of BatchNorm(train)+ReLU: out2k = {S1[c] = sum dyM, S2[c] = sum dyM*xhat} (dyM = dy*[bn(x) > 0]);
 * for SyncBatchNorm all-reduce out2k and use the global count; then dx = gamma*rstd*(dyM - S1/n - xhat*S2/n).
 * d gamma = S2, d beta = S1.  `x` is the pre-normalisation activation, `stats` the forward {sum, sumsq}. */
int contrad_bn_relu_bwd_stats(const float* dy, const float* x, long long M, int K, int ld, const float* stats,
                              float count, const float* gamma, const float* beta, float eps, float* out2k,
                              float* workspace, long long workspace_bytes, contrad_stream_t stream);
int contrad_bn_relu_bwd_apply(const float* dy, const float* x, float* dx, long long M, int K, int ld,
                              const float* stats, float count, const float* gamma, const float* beta, float eps,
                              const float* bstats, contrad_stream_t stream);
/* running_mean / running_var update of nn.BatchNorm2d in train mode (unbiased variance); num_batches_tracked (int64
 * scalar on the device, may be NULL) is incremented by the same launch. */
int contrad_bn_running_update(const float* stats, float count, int K, const float* conv_bias, float momentum,
                              float* running_mean, float* running_var, long long* num_batches_tracked,
                              contrad_stream_t stream);
/* The batch statistics of a train-mode BatchNorm on one device in two launches: stats[2][K] = {sum, sumsq} over the M rows of
 * x (contrad_colstats with with_sq = 1: the same partial sums, lanes and order, bitwise the same stats) and, by the launch
 * that sums the partials, contrad_bn_running_update with count = M (conv_bias / num_batches_tracked may be NULL).
 * SyncBatchNorm needs the reduced stats for its all-reduce BEFORE the running update and keeps the separate calls.
 * workspace: contrad_colstats_workspace_bytes(M, K, 1). */
int contrad_bn_batch_stats(const float* x, long long M, int K, int ld, float* stats, const float* conv_bias,
                           float momentum, float* running_mean, float* running_var, long long* num_batches_tracked,
                           float* workspace, long long workspace_bytes, contrad_stream_t stream);
/* contrad.loss_D_fn's GAN term (training/gan/contrad.py:51-64) on logits[3N] (stride ld): kind 0 nonsat,
 * 1 wgan, 2 hinge, 3 lsgan.  out3 = {loss, mean d_real, mean d_gen}; grad[3N] = d loss / d logits. */
int contrad_gan_d_loss(const float* logits, int ld, int N, int kind, float* out3, float* grad,
                       contrad_stream_t stream);
/* contrad.loss_G_fn (contrad.py:73-82) on logits[N]: kind 0 nonsat, 3 lsgan, other: -mean. */
int contrad_gan_g_loss(const float* logits, int ld, int N, int kind, float* out1, float* grad,
                       contrad_stream_t stream);

/* torch.optim.Adam step (train_gan.py:273-274; no weight decay / amsgrad) fused over up to 64 tensors per
 * launch; `step` is the 1-based step count of these tensors, grad_scale multiplies every gradient first
 * (1/world_size after a sum all-reduce). */
#define CONTRAD_ADAM_MAX_TENSORS 64
#define CONTRAD_ADAM_CHUNK 16384
typedef struct {
  float* p;
  const float* g;
  float* m;
  float* v;
  long long numel;
} contrad_adam_tensor;
typedef struct {
  int n;
  contrad_adam_tensor t[CONTRAD_ADAM_MAX_TENSORS];
  int block_start[CONTRAD_ADAM_MAX_TENSORS + 1]; /* filled by the launcher */
} contrad_adam_batch;
int contrad_adam_step(const contrad_adam_batch* b, int step, float lr, float beta1, float beta2, float eps,
                      float grad_scale, contrad_stream_t stream);
/* The same update with the step-dependent scalars read from DEVICE memory: hyper_dev = {lr / (1 - beta1^t),
 * 1 / sqrt(1 - beta2^t), grad_scale}.  For a D-step captured once into a hipGraph and replayed every iteration (LR
 * warm-up and the bias corrections change per step; launch arguments are frozen at capture). */
int contrad_adam_step_dev(const contrad_adam_batch* b, const float* hyper_dev, float beta1, float beta2, float eps,
                          contrad_stream_t stream);
/* y = a*y + b*x (G EMA `accumulate`, utils.py:130-143) */
int contrad_axpby(float* y, const float* x, long long n, float a, float b, contrad_stream_t stream);
/* dst[0..n) (device) = host_pinned[0..n): a kernel reads device-mapped pinned host memory (hipHostMalloc) directly --
 * the stream-ordered hand-over of the per-step host-side random draws (latents, augmentation parameters). */
int contrad_pull_host(const float* host_pinned, float* dst, long long n, contrad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * SimCLR augmentation, fused (augment/__init__.py:106-122 `simclr()` / `simclr_hq()`):
 * RandomResizeCropLayer + HorizontalFlipLayer (augment/spatial.py:84-148) as ONE bilinear/reflection
 * gather, RandomApply(ColorJitterLayer) (augment/color_jitter.py:16-104, augment/utils.py:6-63),
 * RandomApply(RandomColorGrayLayer) (augment/__init__.py:82-103).  NCHW in, NCHW out, x != y.
 * contrast_first < 0: the colour-op order is read per sample from params[.][15] (hipGraph replay).
 * params[B][CONTRAD_AUG_NPARAM] = {theta00, theta11, theta02, theta12, flip_sign, jitter_mask,
 * f_contrast, f_h, f_s, f_v, gray_mask, blur_mask, cutout_mask, cutout_h_center, cutout_w_center, contrast_first},
 * sampled on the host in the reference's draw order.
 * ---------------------------------------------------------------------------------------------- */
#define CONTRAD_AUG_NPARAM 16
long long contrad_simclr_workspace_bytes(int B, int H, int W);
int contrad_simclr_augment(const float* x, float* y, const float* params, int B, int H, int W,
                           int contrast_first, int has_contrast, float* workspace,
                           long long workspace_bytes, contrad_stream_t stream);
/* Backward of contrad_simclr_augment for the generator step (gradient flows through the augmentation into G,
 * training/gan/contrad.py:73-82, train_stylegan2_contraD.py:138-146): grad_in = d loss / d x given grad_out =
 * d loss / d y.  Bilinear gather transpose, contrast backward, straight-through HSV (augment/color_jitter.py:97-104),
 * gray backward.  Small images (7*H*W + H*H + W*W floats of LDS <= 64 KiB, i.e. CIFAR) run in one block per image and
 * need no workspace; larger images (AFHQ 512x512) take four launches and the workspace sized by the query. */
long long contrad_simclr_augment_bwd_workspace_bytes(int B, int H, int W);
int contrad_simclr_augment_bwd(const float* x, const float* params, const float* grad_out, float* grad_in,
                               int B, int H, int W, int contrast_first, int has_contrast, float* workspace,
                               long long workspace_bytes, contrad_stream_t stream);
/* RandomApply(GaussianBlur) (augment/__init__.py:53-78): separable (2*radius+1)-tap blur with reflect
 * padding on samples whose blur_mask != 0, copy-through otherwise; tmp is a scratch image batch. */
int contrad_gaussian_blur_masked(const float* x, float* tmp, float* y, const float* params,
                                 const float* kernel1d, int B, int H, int W, int radius,
                                 contrad_stream_t stream);
/* RandomApply(CutOut(length)) (augment/spatial.py:152-181; the last stage of `simclr_hq_cutout`, augment/__init__.py:
 * 124-133): in place, y[n,:,i,j] = 0 where |i - h_center| <= (length-1)/2 and |j - w_center| <= (length-1)/2, on the
 * samples whose cutout_mask != 0.  The op is its own backward (a 0/1 mask on the gradient). */
int contrad_cutout_masked(float* y, const float* params, int B, int H, int W, int length, contrad_stream_t stream);
/* Adjoint of contrad_gaussian_blur_masked (the generator step through simclr_hq): grad_in = blur^T(grad_out) on the
 * masked samples (reflect-padding transpose: border contributions fold back), copy-through otherwise. */
int contrad_gaussian_blur_masked_bwd(const float* grad_out, float* tmp, float* grad_in, const float* params,
                                     const float* kernel1d, int B, int H, int W, int radius,
                                     contrad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Baseline training modes (csrc/baseline_aug.hip): the augmentations of `--aug=hfrt|hflip|diffaug`, the consistency
 * penalties of `--penalty=cr|bcr` and the GAN term of training/gan/{std,aug,aug_both}.py.  Images are NCHW fp32
 * contiguous, x != y.  No float atomics: every sum has a fixed order; the backward passes are gathers over pre-images.
 * ---------------------------------------------------------------------------------------------- */
/* HorizontalFlipRandomCrop (augment/spatial.py:14-40; HorizontalFlipLayer :70-93 = max_pixels 0): nearest-neighbour
 * sampling of a flip + integer-shift affine grid with reflection padding, i.e. the index map
 *   y[n,c,i,j] = x[n,c,refl(i + ky), refl((sign > 0 ? j : W-1-j) + kx)],  refl(t) = t < 0 ? -t-1 : (t >= n ? 2n-1-t : t).
 * params[B][CONTRAD_HFRT_NPARAM] = {flip sign (+1 / -1), kx, ky, unused}, kx and ky integers in [-max_pixels, max_pixels].
 * Needs H == W (the reference's shifts are whole pixels only then) and max_pixels < W; -22 otherwise.
 * adjoint != 0: x is d loss / d y, y becomes d loss / d x; every input pixel sums the at most 2 x 2 outputs that read it,
 * rows outer and columns inner, each axis in the order direct, reflected below 0, reflected past n-1. */
#define CONTRAD_HFRT_NPARAM 4
int contrad_hfrt(const float* x, float* y, const float* params, int B, int C, int H, int W, int max_pixels,
                 int adjoint, contrad_stream_t stream);
/* DiffAugment (third_party/diffaug.py) on RGB images, `policy` = bit 1 color | bit 2 translation | bit 4 cutout, applied
 * in this order (the order of the reference's factory, augment/__init__.py:144-145).
 * params[B][CONTRAD_DIFFAUG_NPARAM] = {b, s, c, tx, ty, ox, oy, unused}: b = rand - 0.5 (brightness), s = 2 rand
 * (saturation), c = rand + 0.5 (contrast); tx, ty integer shifts along H, W in [-int(H/8 + .5), int(H/8 + .5)] (W likewise);
 * ox, oy the cutout offsets along H, W.  Entries of stages outside the policy are not read.
 *   u = 2x - 1;  u1 = u + b;  u2 = (u1 - p) s + p, p = mean over the channels of u1;  u3 = (u2 - M) c + M,
 *   M = mean_chw(u2) = mean_chw(u) + b (saturation keeps each pixel's channel mean): ONE per-sample mean of the input;
 *   translation: output (i, j) reads (i + tx, j + ty), 0 outside;  cutout: rows clamp(ox - ch/2 + [0, ch), 0, H-1) x columns
 *   likewise are set to 0, ch = int(H/2 + .5);  y = 0.5 u4 + 0.5 (cut and shifted-out pixels are exactly 0.5).
 * backward != 0: x is d loss / d y and y becomes d loss / d x = 2 gu1, with g3 = 0.5 g masked and un-translated,
 *   gu2 = c g3 + (1 - c) mean_chw(g3), gu1 = s gu2 + (1 - s) mean_c(gu2) (without bit 1: g3 itself).
 * Images of at most 16 KiB (3 x H x W floats; CIFAR) run in one workgroup per image from LDS; larger ones take a
 * partial-sum launch and an apply launch with the workspace of the query. */
#define CONTRAD_DIFFAUG_NPARAM 8
long long contrad_diffaug_workspace_bytes(int B, int H, int W);
int contrad_diffaug(const float* x, float* y, const float* params, int B, int H, int W, int policy, int backward,
                    float* workspace, long long workspace_bytes, contrad_stream_t stream);
/* Consistency term (penalty.py:45-58) of two logit vectors a, b (element strides lda, ldb):
 * out1[0] = lbd0 mean_{i < n0} (a_i - b_i)^2 + lbd1 mean_{n0 <= i < n0 + n1} (a_i - b_i)^2, grad_a / grad_b [n0 + n1] dense
 * = d out / d a, d out / d b.  CR: n1 = 0; bCR: the reals and the fakes of the (2N,1) layout with their two weights. */
int contrad_consistency(const float* a, int lda, const float* b, int ldb, int n0, int n1, float lbd0, float lbd1,
                        float* out1, float* grad_a, float* grad_b, contrad_stream_t stream);
/* contrad_gan_d_loss for the (2N,1) layout of training/gan/{std,aug,aug_both}.py: reals logits[0, N), fakes [N, 2N);
 * kinds and out3 as there, grad[2N]. */
int contrad_gan_d_loss_2n(const float* logits, int ld, int N, int kind, float* out3, float* grad,
                          contrad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The reference's two native ops (models/gan/stylegan2/op/), same tensor contracts.
 * ---------------------------------------------------------------------------------------------- */
/* upfirdn2d_op.upfirdn2d (op/upfirdn2d.cpp:12-23): input [major,in_h,in_w,minor] -> out [major,out_h,out_w,minor],
 * out_h = (in_h*up_y + pad_y0 + pad_y1 - kh)/down_y + 1 (likewise w); zero-insertion upsampling, padding (may be
 * negative), correlation with the flipped FIR kernel [kh,kw], decimation.  The NHWC build passes major = B,
 * minor = C.  Blur / Upsample / Downsample of stylegan2/layers.py:34-92 and their backward / double backward
 * (op/upfirdn2d.py:19-142) are all instances of this one call. */
int contrad_upfirdn2d(const float* input, const float* kernel, float* out, int major, int in_h, int in_w,
                      int minor, int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0,
                      int pad_x1, int pad_y0, int pad_y1, contrad_stream_t stream);
/* The same op with a fused epilogue, used by the discriminator's first-order backward so that no separate elementwise
 * pass exists (the reference runs FusedLeakyReLUFunctionBackward and the residual-gradient adds as their own kernels,
 * op/fused_act.py:20-55, discriminator.py:72-74):  v = upfirdn2d(input) [+ addend];  out = v (if out != NULL);
 * out2 = v * (act_ref > 0 ? gain : slope * gain) (if out2 != NULL).  addend / act_ref / out2 have the output's shape. */
int contrad_upfirdn2d_fused(const float* input, const float* kernel, float* out, int major, int in_h, int in_w,
                            int minor, int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0,
                            int pad_x1, int pad_y0, int pad_y1, const float* addend, const float* act_ref, float slope,
                            float gain, float* out2, contrad_stream_t stream);
/* fused.fused_bias_act (op/fused_bias_act.cpp:11-21): act 1 linear / 3 leaky-relu(alpha); grad 0: y = act(x +
 * bias[(i/step_b) % size_b]) * scale; grad 1: y = x * act'(ref) * scale; grad 2: y = 0.  bias / ref may be NULL
 * where unused.  (FusedLeakyReLU and its first / second backward, op/fused_act.py:20-71.) */
int contrad_fused_bias_act(const float* x, const float* bias, const float* ref, float* y, long long n,
                           int step_b, int size_b, int act, int grad, float alpha, float scale,
                           contrad_stream_t stream);
/* y = a*x + b*z  (ResBlock merge (out + skip)/sqrt(2), stylegan2/discriminator.py:72-74) */
int contrad_lincomb(const float* x, const float* z, float* y, long long n, float a, float b,
                    contrad_stream_t stream);

/* Minibatch-stddev channel (_minibatch_stddev_layer, models/gan/stylegan2/discriminator.py:22-33) on NHWC, with the two
 * backward passes the R1 penalty needs (train_stylegan2.py:106-113 differentiates D's input gradient).  x [B][P][C] dense
 * (P = H*W); the output / gy layout is [B][P][Cp], Cp >= C + 1: channels [0, C) = x, channel C = the group statistic of sample
 * b mod (B / min(B, 4)), channels above = 0 (padding for the conv engine).
 *   mode 0  out [B][P][Cp] = forward(x)
 *   mode 1  out [B][P][C]  = d/dx of <forward(x), gy>                         (gy [B][P][Cp])
 *   mode 2  out [B][P][C], out2 [B][P][Cp] = d/dx, d/dgy of <mode-1 result, h>   (h [B][P][C]) */
int contrad_minibatch_stddev(int mode, const float* x, const float* gy, const float* h, float* out, float* out2,
                             int B, int P, int C, int Cp, contrad_stream_t stream);
/* out[0] = scale * sum_i x[i]^2 in a fixed summation order (r1_loss, train_stylegan2.py:112: grad.pow(2).sum / N) */
long long contrad_sumsq_workspace_bytes(long long n);
int contrad_sumsq(const float* x, long long n, float scale, float* out, float* workspace, long long workspace_bytes,
                  contrad_stream_t stream);
/* y = x * (c * s[0]), s a scalar in device memory (the backward of the line above) */
int contrad_scale_dev(const float* x, const float* s, float c, float* y, long long n, contrad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * StyleGAN2 generator forward helpers (models/gan/stylegan2/generator.py).
 * ---------------------------------------------------------------------------------------------- */
/* Forward-only weight tables of every ModulatedConv2d of the generator in ONE launch (generator.py:52-82): the packed
 * shared weight wp = scale * W in the GEMM layout the conv engine reads, and the demodulation table
 * wsq[c][k] = sum_taps (scale * W[k][c][tap])^2  (demod[n][k] = rsqrt(sum_c style[n][c]^2 wsq[c][k] + 1e-8)).
 * W is ModulatedConv2d.weight[0] = [Cout][Cin][T] as stored (no transposed copy):
 *   transposed == 0: wp[(tap * Cin + c)][k]  (k = cout; a plain conv: contrad_conv2d_fwd),
 *   transposed != 0: wp[(tap * Cout + k)][c] (the upsampling layers' transposed conv = contrad_conv2d_dgrad, and ToRGB =
 *                    contrad_rgb_conv_dgrad).  ldw = leading dimension of wp; columns past the last one are not written.
 * wsq may be NULL (ToRGB does not demodulate). */
#define CONTRAD_MODCONV_MAX_LAYERS 32
typedef struct {
  const float* w;
  float* wp;
  float* wsq;        /* [Cin][Cout] or NULL */
  int Cout, Cin, T, ldw;
  int transposed;
  float scale;
} contrad_modconv_layer;
typedef struct {
  int n;
  contrad_modconv_layer layers[CONTRAD_MODCONV_MAX_LAYERS];
} contrad_modconv_batch;
int contrad_modconv_tables(const contrad_modconv_batch* b, contrad_stream_t stream);
/* Demodulation factors of ALL demodulated layers of one generator forward in one launch (generator.py:62-64):
 * out_l[n][k] = rsqrt( sum_c style_l[n][c]^2 * wsq_l[c][k] + eps ), style_l [B][Cin] (rows contiguous), wsq_l [Cin][K]
 * from contrad_modconv_tables, out_l [B][K].  (Was per layer: a squaring pass, a split-K GEMM + its reduce, add, rsqrt.) */
typedef struct {
  const float* style;
  const float* wsq;
  float* out;
  int Cin, K;
} contrad_demod_layer;
typedef struct {
  int n, B;
  contrad_demod_layer layers[CONTRAD_MODCONV_MAX_LAYERS];
} contrad_demod_batch;
int contrad_modconv_demod(const contrad_demod_batch* b, float eps, contrad_stream_t stream);
/* PixelNorm (stylegan2/layers.py:14-19): y = x * rsqrt(mean_c(x^2) + 1e-8) over rows of [M][K]. */
int contrad_pixelnorm(const float* x, float* y, int M, int K, contrad_stream_t stream);
/* y[n,h,w,c] = x[n,h,w,c] * s[n,c]: weight modulation moved onto the input channels of the shared-weight conv
 * (ModulatedConv2d, generator.py:52-60: (scale * W * style) applied to x == conv(x * style, scale * W)). */
int contrad_nhwc_scale(const float* x, const float* s, float* y, int N, long long HW, int C,
                       contrad_stream_t stream);
/* y = sqrt2 * lrelu_0.2( x * demod[n,k] + noise_w[0] * noise[n,h,w] + bias[k] ), in place allowed:
 * demodulation (generator.py:62-64) + NoiseInjection (:85-94) + FusedLeakyReLU (:113-118) in one pass.
 * demod / noise may be NULL.  post_scale [N,K] (may be NULL): y is additionally multiplied by post_scale[n,k] -- the
 * style vector of the layer that consumes y, i.e. that layer's contrad_nhwc_scale pass folded into this store. */
int contrad_modconv_epilogue(const float* x, const float* demod, const float* noise, const float* noise_w,
                             const float* bias, const float* post_scale, float* y, int N, long long HW, int K,
                             contrad_stream_t stream);
/* The upsampling StyledConv's tail in ONE pass (generator.py:80-83,97-118: Blur after the transposed conv, then
 * demodulation + NoiseInjection + FusedLeakyReLU):  y = modconv_epilogue( upfirdn2d(input; 4x4 FIR, up = down = 1) ),
 * input [N,in_h,in_w,K] -> y [N,out_h,out_w,K]; demod [N,K] / noise [N,out_h,out_w] / post_scale [N,K] may be NULL.
 * post_scale is the NEXT layer's style vector: its weight modulation (contrad_nhwc_scale) rides on this store. */
int contrad_upfirdn2d_modconv(const float* input, const float* kernel, float* y, int N, int in_h, int in_w, int K,
                              int pad_x0, int pad_x1, int pad_y0, int pad_y1, const float* demod, const float* noise,
                              const float* noise_w, const float* bias, const float* post_scale,
                              contrad_stream_t stream);
/* out[n,c] = sum_hw a[n,hw,c] * b[n,hw,c] (b_per_channel != 0) or sum_hw a[n,hw,c] * b[n,hw] (b broadcast over the
 * channels): the gradients of the style vector, the demodulation factor and the noise strength in the backward of
 * ModulatedConv2d / NoiseInjection (generator.py:52-94; the reference gets them from autograd over its grouped
 * conv).  Deterministic two-stage reduction; workspace from contrad_nhwc_dot_workspace_bytes. */
long long contrad_nhwc_dot_workspace_bytes(int N, long long HW, int C);
int contrad_nhwc_dot(const float* a, const float* b, float* out, int N, long long HW, int C, int b_per_channel,
                     float* workspace, long long workspace_bytes, contrad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Linear evaluation head (csrc/linhead.hip): softmax regression on penultimate features F[N,K] (row stride ldf),
 * weights W[C,K] (dense), bias b[C], labels y[N] (int64), 1 <= C <= 128.  Replaces, per iteration of the reference's
 * lin-eval loop (test_lineval.py:79-94: model.linear, CrossEntropyLoss, accuracy(topk=(1,5)), three .item() reads,
 * zero_grad, backward, SGD step; evaluate/classifier.py:11-25,47-67 for the test pass), about twenty launches and
 * three pipeline drains by three launches (two for evaluation) and no host synchronisation.  No float atomics: every
 * sum has a fixed order, results are bitwise repeatable.
 * ---------------------------------------------------------------------------------------------- */
/* Bytes of the workspace of contrad_linhead_fwd (16-byte aligned, caller-allocated); < 0 on bad arguments. */
long long contrad_linhead_workspace_bytes(int N, int K, int C);
/* The launch form of contrad_linhead_fwd for (N, K, C), a pure function of them: number of K-splits whose partial
 * sums are added in order, classes per thread of the logits kernel (ceil(C / 16)), 64-row tiles.  Any output may be NULL. */
int contrad_linhead_plan(int N, int K, int C, int* splits, int* classes_per_thread, int* row_tiles);
/* Launch 1 + 2.  logits[N,C] = F W^T + b (b, logits may be NULL).  With labels: per row the max-subtracted
 * log-sum-exp, loss_n = lse_n - logits[n,y_n], dlogits[N,C] = (softmax - onehot) * dl_scale (NULL: skipped, the
 * evaluation form), and meters4 (device float64, NULL ok) += {sum_n loss_n, top-1 hits, top-5 hits, N}; the label is
 * a top-k hit when fewer than k logits are strictly greater than its logit.  A row whose label is outside [0, C)
 * counts as loss 0, no hit, zero gradient (and still as a sample).  y == NULL: logits only. */
int contrad_linhead_fwd(const float* F, int ldf, const float* W, const float* b, const long long* y, int N, int K,
                        int C, float dl_scale, float* logits, float* dlogits, double* meters4, void* ws,
                        contrad_stream_t stream);
/* Launch 3.  gW[c,k] = sum_n dlogits[n,c] F[n,k], gb[c] = sum_n dlogits[n,c] (n ascending); lr_dev != NULL:
 * W -= lr_dev[0] * gW, b -= lr_dev[0] * gb in place (b may be NULL), the learning rate read from DEVICE memory so that
 * a captured graph follows the MultiStepLR milestones; gradW / gradb != NULL: the gradients are written out. */
int contrad_linhead_wgrad_sgd(const float* F, int ldf, const float* dlogits, int N, int K, int C,
                              const float* lr_dev, float* W, float* b, float* gradW, float* gradb,
                              contrad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * cDDLS sampling (csrc/cddls.hip): the streaming kernels of one class-conditional Langevin step in latent space
 * (the reference's test_gan_sample_cddls.py:57-76) and its noise generator.  Flat tensors of n floats, any n; 16-byte
 * accesses when every pointer is 16-byte aligned.  No allocation, no synchronisation.
 *
 * Noise: Philox4x32-10 keyed by the 64-bit seed, counter (element / 4, step, stream id, 0); the four words give the
 * normals of elements 4q .. 4q + 3 by Box-Muller: radius sqrt(-2 ln u) from word 0 (2), angle 2 pi u from word 1 (3),
 * u = ((word >> 8) + 0.5) 2^-24; elements 0, 2 take the cosine, 1, 3 the sine.  Stream ids: 0 the noise of z, 1 the
 * noise of z2, 2 the initial z2.  state: two device ints {step, arrival counter (0 between launches)}.
 * ---------------------------------------------------------------------------------------------- */
/* out[n] (may be NULL) = the generator's normals, words[n] (may be NULL) = the raw 32-bit words they come from.  The
 * step is step_dev[0] when step_dev != NULL, else `step`.  grid_blocks > 0 forces the grid (the draws do not depend on it). */
int contrad_cddls_normal_fill(float* out, unsigned* words, long long n, long long seed, int stream_id,
                              const void* step_dev, int step, int grid_blocks, contrad_stream_t stream);
/* out[N,F] = (g_head[N,F] + c_row[F]) * (act[N,F] > 0 ? 1 : slope); F % 4 == 0, 16-byte aligned; out may be g_head. */
int contrad_cddls_feature_seed(const float* g_head, const float* c_row, const float* act, float* out, long long N, int F,
                               float slope, contrad_stream_t stream);
/* The same kernel on the two index forms of a residual trunk (d = act > 0 ? 1 : slope; 16-byte aligned pointers):
 * pooled seed  out[N,T,C] = ((g[N,C] + c_row[C]) * (1.0f / T)) * d(act[N,T,C]): the gradient through a mean over T pixels
 *              (NHWC-flat act / out, C % 4 == 0); out must not be g.
 * join         out[n] = (a[n] + b[n]) * d(act[n]), n % 4 == 0: the residual join's backward; out may be a. */
int contrad_cddls_pooled_seed(const float* g, const float* c_row, const float* act, float* out, long long N, int T, int C,
                              float slope, contrad_stream_t stream);
int contrad_cddls_join_bwd(const float* a, const float* b, const float* act, float* out, long long n, float slope,
                           contrad_stream_t stream);
/* Backward of contrad_bn_relu_apply in eval mode (running statistics are constants):
 * dx[r,c] = dy[r,p(c)] * [y[r,p(c)] > 0] * gamma[c] / sqrt(running_var[c] + eps), with y / dy in the layout the apply
 * kernel wrote (row stride ldy; perm_hw > 1: p(ch * perm_hw + hw) = hw * (K / perm_hw) + ch) and dx in x's (row stride
 * ldx).  perm_hw == 1: dx may be dy. */
int contrad_cddls_bn_relu_bwd_eval(const float* dy, const float* y, float* dx, long long M, int K, int ldy, int ldx,
                                   const float* gamma, const float* running_var, float eps, int perm_hw,
                                   contrad_stream_t stream);
/* x = gout + eps * z2; clamp01 != 0: clamped to [0, 1] (the final images). */
int contrad_cddls_compose(const float* gout, const float* z2, float* x, long long n, float eps, int clamp01,
                          contrad_stream_t stream);
/* gx = d(-(d + lbd l))/dx, gout = 0.5 tanh(.) + 0.5 the generator's output.  g_lin = gx * 0.5 (1 - t^2), t = 2 gout - 1;
 * z2 <- z2 - eps / 2 * (eps * gx + z2) + sigma_n sqrt(eps) * n2 in place; n2 = noise[n] when noise != NULL, else stream 1
 * of the generator at step state[0]. */
int contrad_cddls_image_end(const float* gx, const float* gout, float* z2, float* g_lin, long long n, float eps,
                            float sigma_n, const float* noise, long long seed, const void* state,
                            contrad_stream_t stream);
/* z <- clamp(z - eps / 2 * gz + sigma_n sqrt(eps) * n, -1, 1) in place (noise as above, stream 0), then state[0] += 1
 * (state may be NULL with explicit noise). */
int contrad_cddls_latent_update(float* z, const float* gz, long long n, float eps, float sigma_n, const float* noise,
                                long long seed, void* state, contrad_stream_t stream);
/* e[i] = -d[i * ldd] + <feat[i,:F], c_row> + bias_term[0] + 0.5 |z2[i,:P]|^2: the energy of sample i with
 * c_row = -lbd * w_y (in feat's order) and bias_term = -lbd * b_y. */
int contrad_cddls_energy(const float* d, int ldd, const float* feat, const float* c_row, const float* bias_term,
                         const float* z2, float* e, int N, int F, long long P, contrad_stream_t stream);
/* Latent recovery (contrad_amd/recover.py): one more form of the energy, image-end and latent-update kernels, for
 * projecting given images x* onto G by Adam on z.  gout = G(z) and x* are (N, P) rows, phi / phi* (N, F) feature rows.
 * Every call returns -EINVAL before any GPU call on a null required pointer, N / n / P < 1, a feature pointer without its
 * target or residual pointer (or those without it), lr < 0, a beta outside [0, 1) or adam_eps < 0.
 * loss     pix[i] = |gout[i] - x*[i]|^2 / P, feat[i] = |phi[i] - phi*[i]|^2 / F, loss[i] = pix[i] + lambda_feat * feat[i],
 *          resid[i][f] = (2 lambda_feat / F) (phi[i][f] - phi*[i][f]).  phi == NULL (then phi_target and resid too): the
 *          pixel part only, feat[i] = 0.  One block per sample, fixed summation order, no atomics.
 * image end g_lin = ((2 / P) (gout - x*) [+ gx]) * 0.5 (1 - t^2), t = 2 gout - 1; gx may be NULL.  n floats, any n.
 * update   t = state[0] + 1:  m <- beta1 m + (1 - beta1) gz,  v <- beta2 v + (1 - beta2) gz^2,
 *          z <- clamp(z - lr (m / (1 - beta1^t)) / (sqrt(v / (1 - beta2^t)) + adam_eps), -1, 1) in place (the two
 *          corrections in float64, rounded once to fp32), then state[0] += 1 as contrad_cddls_latent_update does. */
int contrad_cddls_recover_loss(const float* gout, const float* target, const float* phi, const float* phi_target,
                               float* resid, float* pix, float* feat, float* loss, int N, int F, long long P,
                               float lambda_feat, contrad_stream_t stream);
int contrad_cddls_recover_image_end(const float* gx, const float* gout, const float* target, float* g_lin, long long n,
                                    long long P, contrad_stream_t stream);
int contrad_cddls_recover_update(float* z, const float* gz, float* m, float* v, long long n, float lr, float beta1,
                                 float beta2, float adam_eps, void* state, contrad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Gradient penalty (csrc/gp.hip): the two device-side pieces of --penalty=gp (the reference's penalty.py:16-42).
 * Rows of chw = C*H*W floats of (N, C, H, W) fp32 NCHW tensors; 16-byte accesses at every 16-byte aligned address (scalar
 * head and tail of a row otherwise).  No float atomics: every sum has a fixed order, results are bitwise repeatable.
 * ---------------------------------------------------------------------------------------------- */
/* xhat[n] = alpha[n] * x[n] + (1 - alpha[n]) * g[n], alpha (N,) on the device.  A row with alpha == 1 is x[n] and a row
 * with alpha == 0 is g[n], bit for bit.  xhat must be neither x nor g. */
int contrad_gp_interpolate(const float* x, const float* g, const float* alpha, float* xhat, int N, long long chw,
                           contrad_stream_t stream);
/* Bytes of the workspace of contrad_gp_penalty (16 for rows of at most 16 KiB, which take one workgroup each with the row
 * staged in LDS; the partial sums of the two-launch form otherwise); < 0 on bad arguments. */
long long contrad_gp_penalty_workspace_bytes(int N, long long chw);
/* norms[n] = ||grad_n||_2, out1[0] = lbd * mean_n (norms[n] - 1)^2, cot[n] = lbd * 2 (norms[n] - 1) / (N * norms[n]) *
 * grad_n = d out1 / d grad; a row with norms[n] == 0 gets cot_n == 0.  cot must not be grad. */
int contrad_gp_penalty(const float* grad, float* norms, float* out1, float* cot, int N, long long chw, float lbd,
                       float* workspace, long long workspace_bytes, contrad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Real-image batches (csrc/data.hip): gather, flip, NHWC -> NCHW and ToTensor in one launch.
 * ---------------------------------------------------------------------------------------------- */
/* dst[b, c, i, j] = (float) src[idx_b, i, (flip_b ? W-1-j : j), c] / 255.0f (correctly rounded: bit-equal to
 * x.float().div(255)).  src uint8 (n, H, W, 3); params (B, 2) fp32 rows {index, flip}: the index is clamped to [0, n)
 * (NaN -> 0), flip != 0 mirrors the row; dst fp32 (B, 3, H, W), 4-byte aligned.  n <= 2^24 (indices are floats).
 * 16-byte stores / dword loads where the addresses allow, scalar head and tail of a row otherwise; bitwise repeatable. */
int contrad_gather_u8_nchw(const unsigned char* src, const float* params, float* dst, int B, int n, int H, int W,
                           contrad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Images for the host (csrc/imagegrid.hip): float NCHW -> uint8 HWC canvas in one launch.
 * ---------------------------------------------------------------------------------------------- */
/* torchvision's make_grid followed by save_image's quantisation.  src fp32 (n, 3, H, W); dst uint8
 * [ymaps * (H + pad) + pad, xmaps * (W + pad) + pad, 3] with ymaps = ceil(n / xmaps): image k starts at row
 * pad + (k / xmaps) * (H + pad), column pad + (k % xmaps) * (W + pad); every other pixel holds pad_value.  Every value is
 * written as trunc(clamp(v * 255 + 0.5, 0, 255)), multiply and add rounded separately (bit-equal to
 * v.mul(255).add_(0.5).clamp_(0, 255).to(uint8)); NaN -> 0.  pad = 0, xmaps = 1: the uint8 (n, H, W, 3) batch.
 * src and dst 4-byte aligned.  Every byte is written once; bitwise repeatable. */
int contrad_image_grid_u8(const float* src, unsigned char* dst, int n, int H, int W, int xmaps, int pad, float pad_value,
                          contrad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Weighted k-nearest-neighbour vote (csrc/knn.hip): top k per row of a similarity matrix, class scores, prediction.
 * An addition of this project (the reference has no kNN evaluator): the probe of Wu et al. 2018 on frozen features.
 * ---------------------------------------------------------------------------------------------- */
/* Bytes of the workspace of contrad_knn_select (0: this form keeps its state in LDS, workspace may then be NULL);
 * < 0 on bad arguments. */
long long contrad_knn_select_workspace_bytes(int M, int n, int k, int C);
/* For every row i of S[M][ldS] (only columns [0, n) are read; labels[n] int64):
 *   neighbours   the first k columns under the total order "value descending, then column ascending"; -0.0 and +0.0
 *                compare equal, NaN compares below every number.  idx[i][0..k) and val[i][0..k) in that order, val the
 *                very floats of S.
 *   scores[i][c] = sum_r [labels[idx[i][r]] == c] * expf(val[i][r] * inv_temp), fp32, added in rank order r = 0..k-1.
 *   pred[i]      the class of the largest score (same order: a NaN score is below every number), the lowest class on
 *                an exact tie.
 * A label outside [0, C) contributes to no score.  1 <= k <= min(n, 1024), 1 <= C <= 1024, ldS >= n; -EINVAL (before
 * any GPU call) on a null pointer, a violated limit or a workspace smaller than contrad_knn_select_workspace_bytes.
 * One launch; no float atomics; every output element is written once; two calls are bitwise equal. */
int contrad_knn_select(const float* S, long long ldS, int M, int n, const long long* labels, int C, int k,
                       float inv_temp, int* idx, float* val, float* scores, int* pred, void* workspace,
                       long long workspace_bytes, contrad_stream_t stream);
/* contrad_knn_select with the query's own column left out: row i of S[M][ldS] is row self0 + i of the bank it is compared
 * with (contrad_prdc_kth's convention: a row chunk passes its first global row) and leaves column e = self0 + i out when
 * self0 >= 0 and e < n; otherwise (self0 < 0, or e >= n) nothing is left out of that row, and self0 < 0 is
 * contrad_knn_select bit for bit.  Exclusion is BY INDEX, whatever the column holds: a NaN or a +inf there is never seen
 * and never written, while a duplicate of the query elsewhere in the bank is a neighbour like any other.  The neighbour
 * order among the columns that remain, val, scores and pred are contrad_knn_select's.  Limits: those of
 * contrad_knn_select, and k <= n - 1 when 0 <= self0 < n (the columns that remain in the shortest row; so n >= 2 there);
 * -EINVAL (before any GPU call) on a null pointer, a violated limit or a workspace smaller than
 * contrad_knn_select_workspace_bytes.  There is no label-free form: a caller without labels passes n zeros, C = 1 and
 * inv_temp = 1.  One launch of the same kernel; no float atomics; every output element is written once; two calls are
 * bitwise equal. */
int contrad_knn_select_loo(const float* S, long long ldS, int M, int n, long long self0, const long long* labels, int C,
                           int k, float inv_temp, int* idx, float* val, float* scores, int* pred, void* workspace,
                           long long workspace_bytes, contrad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Precision / recall / density / coverage on a similarity matrix (csrc/prdc.hip): k-th largest per row, hit counts.
 * An addition of this project (the reference selects by FID): the k-NN manifold metrics of Kynkaanniemi et al. 2019
 * and Naeem et al. 2020 on frozen, L2-normalised features, where "inside the k-NN ball" is "similarity >= threshold".
 * ---------------------------------------------------------------------------------------------- */
/* thr[i], i in [0, M): the k-th largest value of row i of S[M][ldS] over the columns [0, n), column self0 + i left out
 * when it lies in [0, n) (row i of a chunk is global row self0 + i: exclusion is by index, whatever the value there);
 * self0 < 0 leaves nothing out.  The order is contrad_knn_select's: value descending, then column ascending; -0.0 and
 * +0.0 compare equal, NaN compares below every number, so a row with fewer than k numbers yields a NaN.  thr[i] is the
 * very float of the column that holds the k-th place.  1 <= k <= the columns that remain in the shortest row (n - 1 if
 * 0 <= self0 < n, else n), ldS >= n; -EINVAL (before any GPU call) on a null pointer or a violated limit.  One launch,
 * one workgroup per row, no workspace, k not bound by LDS; every output element is written once; bitwise repeatable. */
int contrad_prdc_kth(const float* S, long long ldS, int M, int n, int k, long long self0, float* thr,
                     contrad_stream_t stream);
/* One pass over S[M][ldS] (only columns [0, n) are read), hit(a, t) = a >= t (inclusive; false when either is NaN):
 *   row_hits[i]    = #{j : hit(S[i][j], thr_col[j])}, written (zeroed by a memset node on `stream`, then added to);
 *   col_hits_c[j] += #{i : hit(S[i][j], thr_col[j])};
 *   col_hits_r[j] += #{i : hit(S[i][j], thr_row[i])}.
 * The caller zeroes the two column arrays once and calls once per row chunk.  thr_col == NULL skips row_hits and
 * col_hits_c (both may then be NULL), thr_row == NULL skips col_hits_r; at least one of the two is given.  ldS >= n;
 * -EINVAL (before any GPU call) on a missing pointer or a violated limit.  16-byte loads when S is 16-byte aligned and
 * ldS a multiple of 4, scalar loads otherwise and in a row's tail.  Integer adds only (no float atomics): the sums do not
 * depend on the order of arrival and two calls are bitwise equal. */
int contrad_prdc_count(const float* S, long long ldS, int M, int n, const float* thr_row, const float* thr_col,
                       int* row_hits, int* col_hits_c, int* col_hits_r, contrad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Kernel distance (KID, Binkowski et al. 2018) on a similarity matrix (csrc/kid.hip): the cubic-kernel block sum.
 * An addition of this project (the reference selects by FID): the unbiased MMD^2 under k(a, b) = (gamma a.b + coef0)^3
 * on frozen, L2-normalised features, gamma = coef0 = 1 (contrad_amd/kid.py).  Its values are comparable between
 * evaluations under one encoder file, never with Inception-based KID.
 * ---------------------------------------------------------------------------------------------- */
/* Bytes of workspace contrad_kid_sums needs for an (M, n) block (one float64 partial per workgroup); -EINVAL on M < 1
 * or n < 1. */
long long contrad_kid_sums_workspace_bytes(int M, int n);
/* out[0] = (accumulate ? out[0] : 0) + sum over i < M, j < n, j != self0 + i of (gamma * (double)S[i][j] + coef0)^3 on
 * S[M][ldS] (only columns [0, n) are read: a padding column may hold anything).  self0 < 0 leaves nothing out
 * (contrad_prdc_kth's convention: a row chunk passes its first row); the column is left out by index, whatever it holds.
 * A NaN or inf inside the block propagates.  Every term is formed and added in float64; per-workgroup partials go to
 * `workspace` and are added in one fixed order by a second launch, the old value last and by one thread: no atomics,
 * two calls are bitwise equal.  16-byte loads when S is 16-byte aligned and ldS a multiple of 4, guarded scalar loads
 * otherwise and wherever four columns cross n.  -EINVAL (before any GPU call) on a null S or out, M < 1, n < 1,
 * ldS < n, a non-finite gamma or coef0, a workspace that is null, smaller than the query says or not 8-byte aligned. */
int contrad_kid_sums(const float* S, long long ldS, int M, int n, long long self0, double gamma, double coef0,
                     int accumulate, double* out, void* workspace, long long workspace_bytes, contrad_stream_t stream);
/* contrad_kid_sums with the kernel chosen by `kind`: out[0] = (accumulate ? out[0] : 0) + sum over i < M, j < n,
 * j != self0 + i of k((double)S[i][j]), everything else (layout, exclusion by index, float64 terms and sums, the same
 * workspace query contrad_kid_sums_workspace_bytes, no atomics, two calls bitwise equal) as above.
 *   kind 0: k(s) = (gamma * s + coef0)^3 -- bit for bit contrad_kid_sums;
 *   kind 1: the rational-quadratic mixture on unit vectors, u = 2 - 2 s clamped below at 0 (a NaN stays a NaN; an s
 *           slightly above 1 gives u = 0), k(s) = 1 / sqrt(1 + u) + 1 / (1 + u / 2) + 1 / (1 + u / 4)^2, that is the sum
 *           over alpha in {1/2, 1, 2} of (1 + u / (2 alpha))^-alpha; IEEE sqrt and division only.  gamma and coef0 are
 *           not read but must still be finite.
 * -EINVAL (before any GPU call) on everything contrad_kid_sums refuses and on a kind outside {0, 1}. */
int contrad_mmd_sums(const float* S, long long ldS, int M, int n, long long self0, int kind, double gamma, double coef0,
                     int accumulate, double* out, void* workspace, long long workspace_bytes, contrad_stream_t stream);
/* The sum kernel on two operands (contrad_amd/fd.py: traces, Frobenius norms and the nuclear-norm estimates of the
 * Frechet distance): out[0] = (accumulate ? out[0] : 0) + sum over i < M, j < n of (double)A[i][j] * (double)B[i][j] on
 * A[M][ldA] and B[M][ldB] (only columns [0, n) are read).  Every product is exact in float64 and added in float64; the
 * walk, the workspace (contrad_kid_sums_workspace_bytes(M, n)), the fixed summation order and the second launch are
 * contrad_kid_sums's: no atomics, two calls are bitwise equal.  B may alias A (the sum of squares).  Each operand takes
 * 16-byte loads when it is 16-byte aligned and its leading dimension a multiple of 4, by itself.  A NaN or inf inside
 * either block propagates.  -EINVAL (before any GPU call) on a null A, B or out, M < 1, n < 1, ldA < n, ldB < n, a
 * workspace that is null, smaller than the query says or not 8-byte aligned, an out that is not 8-byte aligned.  This
 * is the only way to the two-operand kind: contrad_mmd_sums refuses every kind outside {0, 1}. */
int contrad_dot_sums(const float* A, long long ldA, const float* B, long long ldB, int M, int n, int accumulate, double* out,
                     void* workspace, long long workspace_bytes, contrad_stream_t stream);
/* The sum kernel with the Gaussian potential of two unit vectors (contrad_amd/contrast.py: the uniformity of Wang &
 * Isola 2020): out[0] = (accumulate ? out[0] : 0) + sum over i < M, j < n, j != self0 + i of exp(-t * u) at
 * u = max(2 - 2 (double)S[i][j], 0), the squared distance (a NaN stays a NaN; an s slightly above 1 gives u = 0 and a
 * term of exactly 1; t = 0 gives the number of cells that count).  u is exact in float64; one float64 multiply and one
 * float64 exp per term.  Layout, exclusion by index, the workspace (contrad_kid_sums_workspace_bytes(M, n)), the fixed
 * summation order and the second launch are contrad_kid_sums's: no atomics, two calls are bitwise equal.  -EINVAL
 * (before any GPU call) on everything contrad_kid_sums refuses (gamma and coef0 apart: there are none) and on a t that
 * is negative, NaN or infinite.  This is the only way to this term: contrad_mmd_sums refuses every kind outside {0, 1}. */
int contrad_gauss_sums(const float* S, long long ldS, int M, int n, long long self0, double t, int accumulate, double* out,
                       void* workspace, long long workspace_bytes, contrad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Sliced Wasserstein distance on Laplacian-pyramid patches (Karras et al. 2018; csrc/eval/swd.hip, contrad_amd/swd.py,
 * DESIGN.md section 22).  An addition of this project: the one sample-quality number here that needs no network.  Image
 * levels are fp32 planes [n * 3][R][R] (plane = image * 3 + channel), values 0 ... 255 as the uint8 set holds them.
 * No entry point uses an atomic: two calls are bitwise equal.
 * ---------------------------------------------------------------------------------------------- */
/* dst[(i * 3 + c)][y][x] = (float)src[i][y][x][c] for the uint8 NHWC set src[n][R][R][3] (exact).  -EINVAL on a null
 * pointer, n < 1, R < 1 or R > 32768. */
int contrad_swd_u8_planes(const void* src_u8, float* dst, long long n, int R, contrad_stream_t stream);
/* One Gaussian pyramid step: coarse[p][y][x] = sum over dy, dx in [-2, 2] of g[dy] g[dx] fine[p][m(2y + dy)][m(2x + dx)]
 * on `planes` planes of R x R (coarse: R/2 x R/2), g = [1 4 6 4 1] / 16 and m the mirror rule d c b | a b c d | c b a
 * (-1 -> 1, -2 -> 2, R -> R - 2, R + 1 -> R - 3).  25 products in fp32 with exact weights, added in the order dy, dx.
 * -EINVAL on a null pointer, fine == coarse, planes < 1, an odd R, R < 4 or R > 32768. */
int contrad_swd_pyr_down(const float* fine, float* coarse, long long planes, int R, contrad_stream_t stream);
/* The Laplacian step in place: fine[p][y][x] -= sum over dy, dx in [-2, 2] of 4 g[dy] g[dx] Z[m(y + dy)][m(x + dx)] with Z
 * the zero-inserted coarse level (Z[2i][2j] = coarse[p][i][j], zero elsewhere), which is never made: the taps on odd
 * coordinates are skipped.  -EINVAL as contrad_swd_pyr_down. */
int contrad_swd_pyr_up_sub(float* fine, const float* coarse, long long planes, int R, contrad_stream_t stream);
/* Bytes of workspace contrad_swd_gather needs for n_desc descriptors; -EINVAL on n_desc < 1. */
long long contrad_swd_gather_workspace_bytes(long long n_desc);
/* Descriptor d < n_desc = n_images * nhoods is the 7 x 7 x 3 patch of image d / nhoods around (cx[d], cy[d]) (a centre
 * outside [3, R - 4] is clamped into it: nothing outside the level is read):
 *   bank[c * 49 + dy * 7 + dx][d] = level[(d / nhoods) * 3 + c][cy[d] + dy - 3][cx[d] + dx - 3]
 * on the transposed bank[148][n_pad], n_pad = n_desc rounded up to a multiple of 4; row 147 and the columns
 * [n_desc, n_pad) are written as zero.  stats[c] / stats[3 + c] (float64): the sum / sum of squares of channel c over
 * every descriptor and position, each value widened (the squares exact) and added in float64 in a fixed order.
 * -EINVAL on a null pointer, n_images < 1, nhoods < 1, R < 7, an n_pad other than the rounded n_desc, a workspace that is
 * null, smaller than the query says or not 8-byte aligned, stats not 8-byte aligned. */
int contrad_swd_gather(const float* level, long long n_images, int R, const int* cx, const int* cy, int nhoods, float* bank,
                       long long n_pad, double* stats, void* workspace, long long workspace_bytes, contrad_stream_t stream);
/* The floats of the sort's LDS tile (a power of two): the row lengths around it are where contrad_swd_sort_rows changes
 * its launch sequence. */
int contrad_swd_sort_tile(void);
/* Sorts each of `rows` rows X[r][0 .. n) (row stride ld >= n) ascending, in place; the values must be finite (zeros of
 * both signs keep some order among themselves).  Nothing at or behind column n is read or written.  -EINVAL on a null X,
 * rows < 1, n < 1, n > 2^30 or ld < n. */
int contrad_swd_sort_rows(float* X, long long ld, int rows, int n, contrad_stream_t stream);
/* Bytes of workspace contrad_swd_absdiff_sums needs; -EINVAL on rows < 1, n < 1 or n > 2^30. */
long long contrad_swd_absdiff_workspace_bytes(int rows, int n);
/* out[0] = (accumulate ? out[0] : 0) + sum over r < rows, i < n of |(double)A[r][i] - (double)B[r][i] + row_offset[r]|
 * (row_offset null: 0), every term formed and added in float64 in a fixed order, the old value last.  Columns >= n are
 * never read.  -EINVAL on a null A, B or out, rows < 1, n < 1, ldA < n, ldB < n, a workspace that is null, smaller than the
 * query says or not 8-byte aligned, an out or row_offset that is not 8-byte aligned. */
int contrad_swd_absdiff_sums(const float* A, long long ldA, const float* B, long long ldB, const double* row_offset, int rows,
                             int n, int accumulate, double* out, void* workspace, long long workspace_bytes,
                             contrad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Radial power spectrum of uint8 images (csrc/spectral/spectrum.hip, contrad_amd/spectrum.py).  An
 * addition of this project: the azimuthally averaged power of the luma, which shows up-sampling artefacts directly.  S is
 * the image side, a power of two in [16, 512]; the half spectrum spec[n][S][S / 2 + 1][2] is numpy.fft.rfft2's layout
 * (u along H, v along W, real then imaginary part).  No entry point takes scratch or uses an atomic: two calls are
 * bitwise equal.
 * ---------------------------------------------------------------------------------------------- */
/* spec[i][u][v] = sum over y, x of Y_i[y][x] exp(-2 pi i (u y + v x) / S), v <= S / 2, of the exact luma
 * Y = (77 R + 150 G + 29 B) / 256 of the uint8 NHWC set src[n][S][S][3], in fp32.  twiddles[j][2] = (cos, -sin)(2 pi j / S),
 * j < S / 2, rounded from float64 by the caller: the device calls no sine.  |spec - exact| <= gamma_m sum |Y| with
 * m = 15 log2 S - 22.  -EINVAL on a null pointer, an S that is no power of two in [16, 512], n < 1 or
 * n > 2^24, src_u8 not 4-byte aligned, twiddles or spec not 8-byte aligned. */
int contrad_spec_rfft2(const void* src_u8, const float* twiddles, float* spec, long long n, int S, contrad_stream_t stream);
/* prof[i][k] = rcount[k] / S^4 * sum over u < S, v <= S / 2 with bin_of[u][v] == k of w(v) |spec[i][u][v]|^2, w = 1 at
 * v = 0 and v = S / 2 and 2 elsewhere (the mean of |F|^2 / S^4 over the full grid's members of bin k when rcount[k] is the
 * reciprocal of their number), squares and sums in float64 in a fixed order.  bin_of[S][S / 2 + 1] (int32) must not
 * decrease along v nor along |fu| and must equal its mirror u -> S - u, as the rounded radius does; only its rows
 * u <= S / 2 are read.  K is the number of bins.  -EINVAL on a null pointer, an S as above, n < 1 or n > 2^24, K outside
 * [S / 2 + 1, S], spec, rcount or prof not 8-byte aligned, bin_of not 4-byte aligned. */
int contrad_spec_radial(const float* spec, const int* bin_of, const double* rcount, double* prof, long long n, int S, int K,
                        contrad_stream_t stream);
/* map[u][v] = (accumulate ? map[u][v] : 0) + sum over i < n of |spec[i][u][v]|^2 / S^4 on the half spectrum, in float64,
 * the images in a fixed order, the old value last: the caller feeds chunks of images and divides by their total number.
 * -EINVAL on a null pointer, an S as above, n < 1 or n > 2^24, accumulate outside {0, 1}, spec or map not 8-byte aligned. */
int contrad_spec_mean_map(const float* spec, double* map, long long n, int S, int accumulate, contrad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Latent-space tools (csrc/latent/latent.hip, contrad_amd/latent.py).  An addition of this project:
 * pairs of latents an exact eps apart, per-layer styles with truncation and mixing, and a pair distance that takes the
 * difference first.  No entry point takes scratch or uses an atomic: two calls are bitwise equal.
 * ---------------------------------------------------------------------------------------------- */
/* out0[i] = the point at t[i] and out1[i] = the point at (double)t[i] + dt of the path from row a[i] to row b[i], all fp32
 * [n][d] dense; every intermediate is float64 and shared by both points, one rounding to fp32 at the store; dt == 0 makes
 * out1 bitwise out0.  mode 0: a + t (b - a).  mode 1 (slerp of Karras et al.): with x^ = x / max(|x|, 1e-300),
 * r = b^ - (a^.b^) a^, theta = atan2(|r|, a^.b^) (never acos), the point is normalize(a^ cos(t theta) + (r / |r|) sin(t theta));
 * where |r| <= (d + 16) 2^-52 (zero to the rounding of the dot product: b = a, b = -a) the point is a^ for every t.
 * -EINVAL on a null pointer, a mode outside {0, 1}, n < 1, n >= 2^31, d < 1, a dt that is not finite, out0 == out1. */
int contrad_latent_pair(const float* a, const float* b, const float* t, double dt, int mode, float* out0, float* out1,
                        long long n, int d, contrad_stream_t stream);
/* out[b][l][:] = w_avg + psi[l] (src - w_avg) in fp32, src = w[b] if l < cross[b] else w2[b]; w, w2 [B][d], w_avg [d], psi [L],
 * cross [B] fp32 (layer counts as floats, the way the generator takes its mixing layers), out [B][L][d].  w2 and cross may
 * both be null (no mixing), w_avg and psi may both be null (no truncation).  A layer with psi[l] == 1, and every layer
 * without psi, holds the bits of the source row.  -EINVAL on a null w or out, B, L or d < 1, w2 without cross or cross
 * without w2, w_avg without psi or psi without w_avg. */
int contrad_latent_styles(const float* w, const float* w2, const float* w_avg, const float* psi, const float* cross, float* out,
                          int B, int L, int d, contrad_stream_t stream);
/* The largest d at which contrad_pair_dist keeps both rows in LDS between its two passes; above it the rows are read twice. */
int contrad_pair_dist_resident_d(void);
/* out[i] = scale * |A^_i - B^_i|^2 in float64, x^ = x / max(|x|, 1e-12), rows A[i] at A + i ldA and B[i] at B + i ldB, d
 * fp32 values each: norms, quotients, differences, squares and sums in float64 in a fixed order, so equal rows give exactly
 * 0.  Columns >= d are never read.  -EINVAL on a null pointer, n < 1, n >= 2^31, d < 1, ldA < d, ldB < d, a scale that is
 * not finite, an out that is not 8-byte aligned. */
int contrad_pair_dist(const float* A, long long ldA, const float* B, long long ldB, long long n, int d, double scale, double* out,
                      contrad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * StyleGAN2 projector (csrc/project/project.hip, contrad_amd/project.py).  An addition of this project:
 * the loss ends of projecting an image onto the generator (Karras et al. 2020, appendix D) under a pixel-pyramid loss.  fp32
 * storage and accumulation, every sum in a fixed order, no atomics: two calls are bitwise equal.  Scratch is a caller-owned
 * array passed with its length in floats (no size query): contents undefined on entry, nothing outside it is written.
 * ---------------------------------------------------------------------------------------------- */
/* pix[l][n] = mean over the 3 (H / 2^l) (W / 2^l) values of pool_l(x[n] - target[n])^2, l < L, pool_l the 2^l x 2^l mean
 * (each level from the one below: ((a + b) + (c + d)) / 4), and gx = d sum_n sum_l lam[l] pix[l][n] / d x
 * = (2 / 3HW) sum_l lam[l] pool_l(x - target)[the tile of the pixel].  x, target, gx fp32 [N][3][H][W] dense; lam: L floats in
 * HOST memory; pix [L][N].  partial: scratch of at least L * N * 3 * (H / rows) floats, rows = T = 2^(L-1) doubled while
 * 2 rows W <= 4096 and 2 rows divides H (L * N * 3 * H / T always suffices).  x == target gives exact zeros everywhere.
 * -EINVAL on a null pointer, L outside [1, 4], N < 1 or N > 65535, H or W not divisible by 2^(L-1), 2^(L-1) W > 8192, a lam
 * that is not finite, gx aliasing an input, a partial that is too short. */
int contrad_proj_image_end(const float* x, const float* target, const float* lam, int L, float* pix, float* gx, float* partial,
                           long long partial_floats, int N, int H, int W, contrad_stream_t stream);
/* g_noise[p] = noise_w[0] * sum_k g_pre[p][k] over the P rows of K channels of an NHWC gradient (the noise map's gradient
 * behind the modulated-conv epilogue); noise_w is read from device memory.  -EINVAL on a null pointer, P < 1 or P > 2^40,
 * K < 1 or K > 65536. */
int contrad_proj_noise_grad(const float* g_pre, const float* noise_w, float* g_noise, long long P, int K, contrad_stream_t stream);
/* The StyleGAN2 noise regulariser of one map set map[N][1][R][R], R a power of two in [4, 1024]: m_0 = map,
 * m_{j+1} = avgpool2(m_j) while the side is above 8 (the first level of side <= 8 is the last: J = 1 for R <= 8, else
 * log2 R - 2), a_j = mean(m_j roll(m_j, 1, W)), b_j = mean(m_j roll(m_j, 1, H)) with circular rolls,
 * reg[n] = sum_j a_j^2 + b_j^2, and g_acc[n][h][w] += scale * d reg[n] / d map[n][h][w] (g_acc is read, then written).
 * scratch: at least N * (sum_{j=1}^{J-1} (R / 2^j)^2 + 2 J ceil(R^2 / 4096) + 2 J) floats, 16-byte aligned: the pooled
 * levels, the partial sums per level, a_j and b_j.  -EINVAL on a null pointer, N < 1 or N > 65535, such an R, a map or scratch
 * off 16 bytes, a scale that is not finite, g_acc == map, a scratch that is too short. */
int contrad_proj_noise_reg(const float* map, float* reg, float* g_acc, float scale, float* scratch, long long scratch_floats, int N,
                           int R, contrad_stream_t stream);
/* In place on map[N][1][R][R], per image: m -= mean(m), then m *= 1 / sqrt(mean(m^2)); a map whose centred square mean is 0
 * becomes all zeros (the paper's code would divide by zero).  The mean is formed about the first element,
 * m[0] + mean(m - m[0]), so a constant map centres to exact zeros.  -EINVAL on a null pointer, N < 1, R no power of two in
 * [4, 1024], a map off 16 bytes. */
int contrad_proj_noise_normalize(float* map, int N, int R, contrad_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CONTRAD_HIP_H */
