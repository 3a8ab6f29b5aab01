/* hrseg.h -- C ABI of libhrseg_hip.so: the MI355X (gfx950) kernels behind the
 * hierarchical-segmentation train-step hot path.
 *
 * The reference (Banksylel/Restrictive-Hierarchical-Semantic-Segmentation) has
 * no FFI layer: its hot path is eager PyTorch ops called from
 * Models/models.py, Metrics/losses.py, Metrics/performance_metrics.py and
 * train.py.  Each entry point below replaces the PyTorch/cuDNN op(s) cited
 * next to it; INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - plain pointers + sizes; every pointer is DEVICE memory owned by the
 *     caller (PyTorch's caching allocator); the library allocates nothing.
 *   - process-wide state (all of it listed here): a thread-local error string;
 *     the tuning overrides of hrseg_tune (plain ints, set them before launching
 *     from several threads); the scratch buffer attached with hrseg_set_scratch
 *     (ONE buffer per process, bound to the device that was current when it was
 *     attached -- launches on another device do not use it -- whose region table
 *     is mutex-protected); the weight-image arena attached with
 *     hrseg_set_weight_image_arena and its host-side table of cached weights (one
 *     per process and device, touched only from the launching thread); the launch
 *     counters of hrseg_launch_count.
 *   - activations are NHWC fp32, addressed as pixel*ld + channel ("ld" =
 *     floats per pixel row, >= C, multiple of 4) so a kernel can read or
 *     write a channel slice of a wider tensor (concat without a copy).
 *   - conv weights are OHWI fp32 = torch channels_last storage of the
 *     reference's [Cout,Cin,kh,kw] parameter.
 *   - logits / probabilities / targets at the API boundary are NCHW fp32
 *     contiguous, as the reference returns them.
 *   - all launches go to `stream` (a hipStream_t); no call synchronises.
 *   - return 0 on success, a negative hrseg_status otherwise;
 *     hrseg_last_error_string() describes the last failure on this thread.
 *   - non-finite values on the activation path stay loud.  Every output element
 *     of a pointwise or reducing kernel has the class (finite, +Inf, -Inf, NaN)
 *     that the same operation gives in torch: ReLU -- on its own, behind a
 *     BatchNorm, a residual add, a resize, a fuse sum or in a convolution
 *     epilogue -- keeps NaN and +Inf and maps -Inf to 0; a 2x2 max-pool window
 *     that holds a NaN gives NaN; the clamp of the grouped KL keeps NaN; softmax
 *     and log-sum-exp give NaN for a NaN or +Inf logit.  One NaN in a training
 *     BatchNorm's input makes the whole channel and its running statistics NaN.
 *     A resize gives a non-finite output wherever the poisoned input has a
 *     non-zero interpolation weight (a zero-weight tap may or may not).  The
 *     max|dy| recorders (hrseg_absmax, hrseg_bn_bwd_t.dy_absmax, hrseg_head_bn_t.
 *     dy_absmax, hrseg_bilinear_bwd_multi) report NaN as +Inf.  No forward kernel
 *     turns a non-finite value into a finite one except where torch does
 *     (relu(-Inf) = 0).  One departure from torch, in the backward: the ReLU
 *     mask is [z > 0], so the incoming gradient of an element whose activation
 *     is NaN is zeroed (hrseg_relu_bwd, hrseg_bn_bwd_group, the relu_mask byte,
 *     the fused head backward), where torch's threshold_backward passes it.  The
 *     activation itself is NaN and loud, and a NaN in a training BatchNorm's
 *     channel makes that channel's backward sums and dy NaN regardless.  So a
 *     poisoned activation reaches the loss and the flat gradient, where
 *     FusedAdamW(skip_nonfinite) voids the step.
 *     (tests/nonfinite_ref.py states this per operation.)
 */
#ifndef HRSEG_H
#define HRSEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* hrseg_stream_t; /* hipStream_t */

enum hrseg_status {
  HRSEG_OK = 0,
  HRSEG_ERR_INVALID_ARG = -1,
  HRSEG_ERR_LAUNCH = -2,
  HRSEG_ERR_UNSUPPORTED = -3,
};

const char* hrseg_last_error_string(void);
int hrseg_abi_version(void);

/* ------------------------------------------------------------------ convolution
 * Replaces nn.Conv2d as used at Models/models.py:113,116 (UNet 3x3+bias),
 * :322-324 conv3x3, :364-370 Bottleneck 1x1/3x3, :483-511 fuse 1x1 / 3x3 s2,
 * :579-582 stem, :614 shared_head 1x1, :656 downsample, :690,:701 transitions.
 * k in {1,3}, stride in {1,2}, pad = (k-1)/2.  Cin, Cout multiples of 16
 * (implicit GEMM on v_mfma_f32_16x16x4_f32) except the stem-style Cin<=4 layer,
 * which the forward and weight-gradient calls route to direct kernels.       */
/* Arithmetic of the contraction (operands and results are fp32 in memory in every mode):
 *   F32     fp32 operands on v_mfma_f32_16x16x4_f32 (exact fp32 products)
 *   BF16X3  each operand split exactly into 3 bf16 pieces, the 6 largest of the 9 piece products on
 *           v_mfma_f32_16x16x32_bf16 with fp32 accumulation: fp32-grade (dropped terms < 2^-24 relative)
 *           at 16/6 of the fp32 matrix rate
 *   BF16X2  2 pieces, 3 products (operand error 2^-16)
 *   BF16    operands rounded to bf16, fp32 accumulation (BASELINE configs[4] arithmetic)
 *   AUTO    fp32-grade results from the faster family per problem: FP16X2 for forward / data-gradient problems of
 *           at least 8192 output pixels, for every 3x3 stride-1 problem the wave-specialised kernels take (>= 96
 *           tiles) and for every weight gradient; F32 for the remaining small problems
 *   FP16X2  each operand scaled by a power of two and split into 2 fp16 pieces (22 significand bits), the 3
 *           largest piece products on v_mfma_f32_16x16x32_f16 with fp32 accumulation: operand error 2^-22 at
 *           half the matrix work of BF16X3.  Weights are scaled by 2^8, gradient operands by 2^14 / |max|
 *           (`grad_absmax`, written by hrseg_bn_bwd_group); activations are NOT scaled and NOT clamped:
 *           |x| <= 65504 is exact to 22 bits, up to ~1.3e5 the low piece absorbs the excess, beyond that the
 *           result is Inf / NaN (loud, never a silently saturated value); NaN / Inf inputs propagate.  A caller
 *           that cannot bound its activations checks them with hrseg_absmax and passes F32 (ops.py does so in
 *           deterministic mode).                                                                             */
enum hrseg_conv_precision { HRSEG_CONV_F32 = 0, HRSEG_CONV_BF16X3 = 1, HRSEG_CONV_BF16X2 = 2, HRSEG_CONV_BF16 = 3, HRSEG_CONV_AUTO = 4,
                            HRSEG_CONV_FP16X2 = 5 };
typedef struct {
  int B, Hi, Wi, Cin, ldx; /* input  x[B,Hi,Wi,Cin], row stride ldx   */
  int Ho, Wo, Cout, ldy;   /* output y[B,Ho,Wo,Cout], row stride ldy  */
  int ksize, stride;       /* 1 or 3 ; 1 or 2                          */
  int precision;           /* hrseg_conv_precision                     */
  const float* grad_absmax; /* FP16X2, data / weight gradient: DEVICE array of 64 floats whose maximum is max|dy|
                               of the gradient operand (hrseg_bn_bwd_t.dy_absmax writes it; NULL: unscaled --
                               gradients below 6e-5 then lose precision)                                   */
  const float* residual;    /* forward only, fused epilogue for inference with BatchNorm folded into the weights       */
  int ldr, relu;            /* (hrseg_bn_fold): y = relu?(conv(x, w) + bias + residual[pixel*ldr + channel]); residual
                               may be NULL; zero-initialised fields = plain convolution                               */
  double* stat_partial;     /* forward only, optional: DEVICE buffer of 256 * 2 * Cout doubles.  A kernel that can (the
                               wave-specialised 3x3 kernels) leaves the BatchNorm partial sums of its OUTPUT there -- row r
                               = [sum y over the pixels block r produced][sum y^2], per output channel -- the layout
                               hrseg_bn_fwd_t.partial has with nchunks = *stat_rows: the caller then runs hrseg_bn_fwd_group_
                               phases without the statistics phase (phases 6).  The rows are complete sums in a fixed order
                               per block, but the blocks' LDS atomics meet in any order (last bits of the fp64 sums vary): not
                               offered in deterministic mode                                                              */
  int* stat_rows;           /* HOST pointer, out (set by the call, synchronously): rows written to stat_partial; 0 = the
                               kernel that ran produces no statistics (run the statistics phase).  Required with stat_partial */
  int x_split;              /* forward / weight gradient: x is stored PRE-SPLIT (hrseg_bn_fwd_t.z_split wrote it: per 4 channels the
                               dwords {hi01, hi23, lo01, lo23} of the fp16x2 split).  Only the wave-specialised forward kernels and
                               the nine-tap weight gradient read that form: ask hrseg_conv_x_split_ok first; a call that cannot
                               take those kernels FAILS (HRSEG_ERR_UNSUPPORTED), it never reads the bytes as fp32           */
  int w_persistent;         /* forward / data gradient: the weight operand is a parameter inside one of the ranges registered
                               with hrseg_set_weight_image_arena, and the caller calls hrseg_weight_images_refresh after every
                               change of those parameters: the kernels that read pre-split weight images then take the cached
                               image instead of writing one in front of the launch.  0 (default): never cached            */
} hrseg_conv_shape_t;

/* 1 when the forward call hrseg_conv_fwd_group(n, shapes) would run the wave-specialised kernels for EVERY problem and
 * hrseg_conv_wgrad_group_ws would run the nine-tap kernel for all of them, i.e. when the producer of x may store it pre-split
 * (x_split); 0 otherwise.  Pure host logic on the shapes, the attached scratch / tuning state and the precision.           */
int hrseg_conv_x_split_ok(int n, const hrseg_conv_shape_t* shapes);
/* all conv weights of a flat parameter buffer at once: `table` (device, 8 ints per entry) lists one
 * 32x32 (cout,cin) tile of one tap per entry {slot offset, Cout, taps, Cin, co0, ci0, tap, 0}; the
 * transposed weight of a slot is written at the same offset of flat_t. */
int hrseg_weight_transpose_all(const float* flat, float* flat_t, const int* table, int nentries,
                               hrseg_stream_t stream);
/* The convolution calls: n >= 1 independent convolutions (a single layer is a group of one; the parallel
 * HRNet branches, models.py:524-525; the fuse paths of a module, :483-511) in ONE launch when 2 <= n <= 8
 * and they can share a kernel instance (channel counts all multiples of 48 or all of 64), else n separate
 * launches; a stride-2 data gradient is one launch per problem (its four parity classes grouped).  Problems
 * of one data-gradient call must write distinct dx buffers.  Pointer arrays are HOST arrays.
 *   fwd:   y = conv(x, w) + bias.  w: [Cout][k*k][Cin]; `bias`, or any bias[i], may be NULL.
 *   dgrad: dx = conv_transpose(dy, w) (+ dx where accumulate[i]).  wt: [Cin][k*k][Cout]
 *          (hrseg_weight_transpose of w).  Shape as the forward conv's.
 *   wgrad: dw += x (*) dy  (fp32 atomics; dw is [Cout][k*k][Cin] and must hold the running gradient,
 *          zeroed by the caller at the start of a step). */
int hrseg_conv_fwd_group(int n, const float* const* x, const float* const* w,
                         const float* const* bias, float* const* y,
                         const hrseg_conv_shape_t* shapes, hrseg_stream_t stream);
int hrseg_conv_dgrad_group(int n, const float* const* dy, const float* const* wt, float* const* dx,
                           const int* accumulate, const hrseg_conv_shape_t* shapes,
                           hrseg_stream_t stream);
int hrseg_conv_wgrad_group(int n, const float* const* x, const float* const* dy, float* const* dw,
                           const hrseg_conv_shape_t* shapes, hrseg_stream_t stream);
/* Weight gradients with a caller-provided workspace: full 3x3 stride-1 problems in a split-precision mode
 * (channels multiples of 48, or of 64) run the nine-tap kernel -- per-block partial sums written with plain
 * stores into the workspace, then added to dw in a fixed order (no atomics: bit-reproducible).
 * hrseg_conv_wgrad_workspace_bytes returns the size that path needs for the n problems (0: it does not
 * apply); with a NULL / too small workspace, or other shapes, the call is hrseg_conv_wgrad_group. */
size_t hrseg_conv_wgrad_workspace_bytes(int n, const hrseg_conv_shape_t* shapes);
int hrseg_conv_wgrad_group_ws(int n, const float* const* x, const float* const* dy, float* const* dw,
                              const hrseg_conv_shape_t* shapes, void* workspace, size_t workspace_bytes,
                              hrseg_stream_t stream);
/* launches issued so far by kernel family ("ws", "ws_group", "patch_sp", "sp_im2col", "sp_pgroup", "sp_group", "f32",
 * "f32_group", "wgrad_sp", "wgrad_sp_group", "wgrad_f32", "wgrad_f32_group", "wgrad9", "small_cin", "sp_wide"; NULL = all); reset != 0
 * zeroes what it returns.  "ws_canvas" counts PROBLEMS (not launches, not part of the NULL total) that a "ws" / "ws_group"
 * launch tiled as one canvas of side-by-side images, "wgrad_sp_t5" the "wgrad_sp" launches on 80 x 80 tiles ("wgrad_sp_wide": the wide-tile weight-gradient kernel, a family of its own).  The parity tests use it to prove which kernels a case ran.
 * "augment_image" / "augment_targets" (the input pipeline) and "decode_labels" (the output pipeline, 1 launch per
 * hrseg_decode_labels call) and "score_labels" (the scoring pipeline, 1 launch per hrseg_score_labels call), "decode_views"
 * and "flip_views" (test-time augmentation, 1 launch per hrseg_decode_views / hrseg_flip_views call), "window_crops" and
 * "decode_windows" (sliding-window inference, 1 launch per hrseg_window_crops / hrseg_decode_windows call) and "ohem" (online hard
 * example mining: 1 launch per hrseg_ohem_scores, 7 per hrseg_ohem_select, 1 per hrseg_loss_partials_ohem / hrseg_loss_bwd_ohem call),
 * "label_components" / "filter_components" (post-processing) and "score_boundaries" (boundary scoring, HRSEG_SCORE_BOUNDARIES_LAUNCHES
 * per hrseg_score_boundaries call), "score_instances" (instance scoring) and "score_calibration" (calibration scoring, 1 launch
 * per hrseg_score_calibration call), "decode_hedged" (the hedged decode, 1 launch per hrseg_decode_hedged call) and "mix" (the
 * mixing augmentation, 1 launch per hrseg_mix_* call) and "border_weights" (2 launches per hrseg_border_weights call) and "consensus_labels" (1 launch per hrseg_consensus_labels call) and "tree_kl" (1 launch per hrseg_tree_kl / hrseg_tree_kl_bwd call) are families of their own, outside the NULL total and the convolution
 * counts. */
long hrseg_launch_count(const char* family, int reset);
/* tile-plan overrides and A/B switches for the sweep tools under tools/ (value 0 = automatic plan).  Keys: igemm_wtm,
 * igemm_kc, igemm_db, igemm_ksplit, group_wtm, wgrad_pix, wgrad_db, wgrad_blocks, wgrad_group_mult,
 * wgrad_group_min, wgrad_group_max (fp32 kernels); sp_wtm, sp_wtn, sp_ksplit, sp_patch, sp_persist (split-precision
 * kernels); sp_ws (0: never use the wave-specialised 3x3 kernels), sp_ws_n48 (0: 48-channel tilings stay on the
 * block-synchronous kernels), sp_ws_waste (accepted tile padding, percent), sp_ws_bf16 (0: the BF16 arithmetic stays off the wave-specialised kernels), small_cin3 (0: the 3-channel first layer on the generic
 * Cin <= 8 kernels), sp_ws_canvas (0: tile every image on its own, never the batch as one
 * canvas), sp_img (0: block-synchronous kernels
 * split their weights on the fly); wgrad9 (0: never the nine-tap weight gradient), wgrad9_blocks (its target block count per problem; wgrad9_blocks1 .. wgrad9_blocks4: the same for launches of 1 .. 4 problems); wgrad_group_sp (0: grouped tap-per-block
 * weight gradients stay on the fp32 kernel), wgrad_sp_t5 (0: no 80 x 80 tiles for the wide layers), wgrad_sp_wide (0: never the wide-tile weight-gradient body); deterministic (1: single-adder
 * reductions everywhere); routing thresholds sp_ws_min_tiles (96), auto_min_pixels (8192), sp_patch_min_tiles (192): the
 * parity tests lower them so that small cases run the kernels of the headline sizes -- csrc/conv.hip, hrseg_tune.  Unknown key: HRSEG_ERR_INVALID_ARG. */
int hrseg_tune(const char* key, int value);
/* Persistent weight images.  The wave-specialised kernels read their weights from a pre-split image (4 bytes per weight); by
 * default a small kernel writes it in front of every launch.  With an arena attached -- DEVICE memory the caller owns: `arena`
 * (256-byte aligned, at least 1 MiB; 8 bytes per parameter covers forward and data-gradient images of a whole model) and
 * `table` (256-byte aligned, 40 bytes per cached weight) -- the images of weights flagged hrseg_conv_shape_t.w_persistent that lie
 * in [lo0, hi0) or [lo1, hi1) (the parameter buffer and its transposed copy) are kept: written on first use, and ALL rewritten
 * by ONE launch of hrseg_weight_images_refresh, which the caller issues whenever those parameters changed (once per train step)
 * before the convolutions.  Re-attaching (or (NULL, 0, ...)) forgets every cached image.  One arena per process, bound to the
 * device that was current when it was attached.  Reference ops replaced: none (an implementation detail of nn.Conv2d here). */
int hrseg_set_weight_image_arena(void* arena, size_t bytes, void* table, size_t table_bytes, const float* lo0, const float* hi0,
                                 const float* lo1, const float* hi1);
int hrseg_weight_images_refresh(hrseg_stream_t stream);
/* Scratch memory for the convolution launches (device, 256-byte aligned, at least 1 MiB; 256 MiB covers every layer
 * of the reference's models): the wave-specialised fp16x2 kernels of the wide 3x3 stride-1 layers read their weights
 * from a pre-split image (4 bytes per weight) that a small kernel writes there right before each launch, on the same
 * stream (up to eight streams get an eighth of the buffer each, as a ring; the images of one grouped launch are reserved
 * together, so the ring never wraps inside a group; a group whose images do not fit a region, a ninth stream, or a launch
 * on another device than the one current at attach time takes the block-synchronous kernels).  The buffer stays the caller's and must outlive the launches; (NULL, 0) detaches it.
 * Without it those layers run the block-synchronous kernels: same results, slower. */
int hrseg_set_scratch(void* ptr, size_t bytes);
/* wt[ci][t][co] = w[co][t][ci] */
int hrseg_weight_transpose(const float* w, float* wt, int Cout, int taps, int Cin,
                           hrseg_stream_t stream);

/* ------------------------------------------------------------------ batch norm
 * Replaces nn.BatchNorm2d / SyncBatchNorm-without-process-group in training
 * mode (Models/models.py:114,117; bn_helper.py:4-11; BN_MOMENTUM :318) fused
 * with the ReLU / residual add that follows it (:115,118,345,353-354,542).
 * One implementation: the grouped forms below, which take n = 1 for a single
 * problem and a phase mask for a single launch of the three.                   */
/* inference: BatchNorm (running statistics) folded into the convolution in front of it -- w_out[co][:] = w[co][:] * s,
 * b_out[co] = (bias[co] - running_mean[co]) * s + beta[co] with s = gamma[co] / sqrt(running_var[co] + eps); `row` =
 * k*k*Cin floats per output channel (OHWI), bias may be NULL.  With hrseg_conv_shape_t.residual / relu the whole
 * conv + BN (+ residual) (+ ReLU) of models.py:113-118, 332-354 is then ONE launch. */
int hrseg_bn_fold(const float* w, const float* bias, const float* gamma, const float* beta, const float* running_mean,
                  const float* running_var, float eps, int Cout, int row, float* w_out, float* b_out,
                  hrseg_stream_t stream);
/* n (1..8) independent BatchNorm problems in three launches (statistics, finalize, apply; eval: coefficients,
 * apply) resp. (reduce, finalize, apply) for the backward.
 * Forward: partial[nchunks][2][C] (double) receives the per-channel sums of y and y*y over pixel chunks; the finalize
 * reduces them, writes mean, rstd, scale, shift ([4][C] fp32 in `coef`), updates the running statistics (momentum,
 * unbiased variance) and num_batches_tracked if given; the apply is z = relu?( y*scale + shift (+ residual) ).
 * Backward: g = dz * (z>0 if relu); partial sums of g and g*xhat; dgamma += sum g*xhat, dbeta += sum g (if not NULL);
 * dy = gamma*rstd*(g - mean_g - xhat*mean_gx); optionally dres (+)= g. */
typedef struct {
  const float* y; int ldy; long npix; int C;       /* conv output [npix][C]                      */
  const float* gamma; const float* beta;
  float* running_mean; float* running_var; int64_t* num_batches_tracked;   /* updated in training  */
  float momentum, eps;
  const float* residual; int ldr; int relu;          /* z = relu?(bn(y) + residual)                */
  float* z; int ldz;
  float* coef;                                       /* out: [4][C] mean, rstd, scale, shift       */
  double* partial; int nchunks;                      /* scratch nchunks*2*C doubles (training)     */
  int stat_div;                                      /* training: the tensor holds stat_div identical
                                                        copies of one pass's images (batched level
                                                        passes); the unbiased-variance factor uses
                                                        npix/stat_div (0 or 1 = plain)               */
  int stat_updates;                                  /* training: times the batch statistics enter
                                                        the running averages / num_batches_tracked
                                                        (0 or 1 = once; L = de-duplicated level
                                                        passes, see Models/models.py)               */
  unsigned char* relu_mask;                          /* optional out, [npix][C/4] bytes: bit j of byte (pixel, q) =
                                                        channel 4q+j passed the ReLU; the backward of a layer WITH a
                                                        residual reads it (hrseg_bn_bwd_t.relu_mask) instead of z    */
  int z_split;                                       /* != 0: z is written PRE-SPLIT for fp16x2 convolutions (per 4
                                                        channels {hi01, hi23, lo01, lo23}, same 16 bytes): only for a
                                                        tensor whose every reader takes hrseg_conv_shape_t.x_split */
  int residual_split;                                /* != 0: `residual` is stored pre-split (z_split of the launch that
                                                        wrote it); the apply phase adds hi + lo, i.e. the fp32 value
                                                        rounded to the 22 bits the convolutions multiply            */
  int stat_ranks;                                    /* cross-rank statistics (opt-in synchronised BN): the
                                                        partial sums were all-reduced over this many ranks of
                                                        equal shards between the statistics and the finalize
                                                        phase, so the statistics cover stat_ranks*npix pixels
                                                        (0 or 1 = this rank only, the reference's behaviour)  */
} hrseg_bn_fwd_t;
int hrseg_bn_fwd_group(int n, const hrseg_bn_fwd_t* problems, int training, hrseg_stream_t stream);
/* the same in phases (bit 0 statistics, bit 1 finalize / eval coefficients, bit 2 apply; 7 = all): a caller that
 * synchronises BatchNorm statistics across ranks runs phase 1, all-reduces `partial`, then runs phases 2|4 with
 * stat_ranks set (the reference's SyncBatchNorm would do this WITH a process group; it never has one).
 * A problem needs only what its phases touch: y with bit 0 (training) or bit 2; z, ldz with bit 2; partial / nchunks in
 * training with bit 0 or 1; the running statistics in eval with bit 1; coef always. */
int hrseg_bn_fwd_group_phases(int n, const hrseg_bn_fwd_t* problems, int training, int phases, hrseg_stream_t stream);
typedef struct {
  const float* dz; int lddz; const float* z; int ldz; int relu;   /* relu with z == NULL: the forward had
                                                        no residual, the mask is recomputed from y    */
  const float* y; int ldy; const float* coef;
  float* dgamma; float* dbeta;                       /* += (may be NULL)                            */
  float* dy; int lddy;                               /* out (may alias dz)                          */
  float* dres; int lddres; int dres_accumulate;      /* residual gradient (=|+=) g, or NULL         */
  long npix; int C;
  double* partial; int nchunks;                      /* scratch (nchunks+max(nseg,1))*2*C doubles   */
  float* dy_absmax;                                  /* optional DEVICE array of 64 floats (reset by the call):
                                                        slot (block % 64) receives the max|dy| of its blocks;
                                                        feeds hrseg_conv_shape_t.grad_absmax              */
  int nseg;                                          /* > 1: npix is nseg equal segments (the batched
                                                        level passes), each normalised on its own: the
                                                        batch means of the backward are per segment;
                                                        must divide nchunks and npix (0 or 1 = plain)  */
  const unsigned char* relu_mask;                    /* optional: the forward's ReLU mask bytes; given, neither z is
                                                        read nor the mask recomputed (4 B per element less per pass
                                                        on layers with a residual)                                  */
  int sum_ranks;                                     /* cross-rank statistics: the partial sums were all-reduced
                                                        over this many ranks between the reduce and the finalize
                                                        phase; the finalize divides them by it, so that the batch
                                                        means are global and dgamma / dbeta receive this rank's
                                                        share (0 or 1 = this rank only)                      */
} hrseg_bn_bwd_t;
int hrseg_bn_bwd_group(int n, const hrseg_bn_bwd_t* problems, int eval_mode, hrseg_stream_t stream);
/* phases: bit 0 reduce, bit 1 finalize, bit 2 apply (7 = all), see hrseg_bn_fwd_group_phases */
int hrseg_bn_bwd_group_phases(int n, const hrseg_bn_bwd_t* problems, int eval_mode, int phases, hrseg_stream_t stream);

/* ------------------------------------------------------------------ pooling / resampling / glue
 * nn.MaxPool2d(2) (models.py:140); bilinear align_corners=True resize
 * (nn.Upsample :156, F.interpolate :536-539,:746,:757,:766,:776) incl. the
 * zero pad of `up` (:166-170) and the channel concat (:172,:747).            */
int hrseg_maxpool2_fwd(const float* x, int ldx, float* y, int ldy, int B, int Hi, int Wi, int C,
                       hrseg_stream_t stream);
int hrseg_maxpool2_bwd(const float* x, int ldx, const float* dy, int lddy, float* dx, int lddx,
                       int accumulate, int B, int Hi, int Wi, int C, hrseg_stream_t stream);
/* out[b, py+oy, px+ox, :] (op)= bilinear(in)[oy,ox]; region outside the
 * placed image is zero-filled when !accumulate. out image is Hout x Wout,
 * the resized image Hr x Wr placed at (py,px). relu applied after the add. */
int hrseg_bilinear_fwd(const float* in, int ldin, int B, int Hi, int Wi, int C, float* out,
                       int ldout, int Hout, int Wout, int Hr, int Wr, int py, int px,
                       int align_corners, int accumulate, int relu, hrseg_stream_t stream);
int hrseg_bilinear_bwd(const float* dout, int lddout, int B, int Hi, int Wi, int C, float* din,
                       int lddin, int Hout, int Wout, int Hr, int Wr, int py, int px,
                       int align_corners, int accumulate, hrseg_stream_t stream);
/* max|x| of an NHWC tensor: slot (block % 64) of the 64-float DEVICE array out64 (zeroed by the caller) is raised to
 * the maximum of its blocks; NaN counts as +Inf.  Range check in front of FP16X2 convolutions (see above). */
int hrseg_absmax(const float* x, int ldx, long npix, int C, float* out64, hrseg_stream_t stream);
/* HRNet fuse sum (models.py:527-542) in one pass: out = relu?( sum of n_same (1..4) same-resolution NHWC terms + sum of
 * n_low (0..3) terms bilinearly resized from Hi[j] x Wi[j] to H x W ); HOST arrays of pointers / strides / sizes */
int hrseg_fuse_sum(int n_same, const float* const* same, const int* ld_same, int n_low, const float* const* low,
                   const int* ld_low, const int* Hi, const int* Wi, float* out, int ldo, int B, int H, int W, int C,
                   int align_corners, int relu, hrseg_stream_t stream);
/* The HRNet head's 1x1 convolution at branch resolution (models.py:743-747 + the first shared_head layer).  Bilinear
 * weights do not depend on the channel and sum to one, so conv1x1(cat_j up(x_j)) + b = W_0 x_0 + sum_j up(W_j x_j) + b with
 * W_j the column block of the weight that reads branch j: the convolutions run at each branch's own size, 1/8 of the
 * multiply-adds, and the concatenated tensor never exists.  The four entry points below are the glue around them.
 *
 * hrseg_head_mix: y (B x H x W x C, holding t_0 = W_0 x_0) += sum of n_low (0..3) terms low[j] (B x Hi[j] x Wi[j] x C)
 * bilinearly resized to H x W (hrseg_fuse_sum's expression), then + bias[C] (may be NULL), in place.  partial (may be NULL):
 * [nchunks][2][C] doubles, the per-chunk sums of y and y^2 in the layout hrseg_bn_fwd_t.partial / nchunks of the finalize
 * phase: no statistics pass over y is needed.  Chunk k covers pixels [k * ceil(npix / nchunks), ...); fixed order, no
 * atomics: the same bits every run.  HOST arrays of pointers / strides / sizes. */
int hrseg_head_mix(float* y, int ldy, const float* bias, int n_low, const float* const* low, const int* ld_low,
                   const int* Hi, const int* Wi, int B, int H, int W, int C, int align_corners, double* partial,
                   int nchunks, hrseg_stream_t stream);
/* its backward: the transpose of the bilinear resize of dout (B x Hout x Wout x C) onto n (1..3) targets din[j]
 * (B x Hi[j] x Wi[j] x C, overwritten) in one launch; each target equals hrseg_bilinear_bwd of the same dout up to the
 * order of the additions and of the two weight products (large gradients stream dout through LDS and add
 * wy * (sum wx * g), csrc/elem.hip).  No float atomics: the same bits every run, and for every setting of hrseg_tune
 * bwd_multi_slab / bwd_multi_bands that keeps the shape on one body.  absmax (may be NULL): [n][64] floats zeroed by the
 * caller, row j receives max|din[j]| as hrseg_absmax leaves it (the FP16X2 gradient scale of the convolutions that
 * follow).  HOST arrays. */
int hrseg_bilinear_bwd_multi(const float* dout, int lddout, int B, int Hout, int Wout, int C, int n,
                             float* const* din, const int* lddin, const int* Hi, const int* Wi, int align_corners,
                             float* absmax, hrseg_stream_t stream);
/* column blocks of a weight [rows = Cout * taps][Cin]: n (1..8) blocks of widths[j] input channels (multiples of 4 that
 * sum to Cin; HOST array) are copied to `blocks`, laid end to end as contiguous [rows][widths[j]] matrices (block j
 * starts at rows * (widths[0] + ... + widths[j-1]) floats); scatter_add is the reverse with dw += (the gradient). */
int hrseg_weight_cols_gather(const float* w, int rows, int Cin, int n, const int* widths, float* blocks,
                             hrseg_stream_t stream);
int hrseg_weight_cols_scatter_add(const float* blocks, int rows, int Cin, int n, const int* widths, float* dw,
                                  hrseg_stream_t stream);
/* out = relu?(a + b) ; strided channel copy ; masked relu backward */
int hrseg_add(const float* a, int lda, const float* b, int ldb, float* out, int ldo, int relu,
              long npix, int C, hrseg_stream_t stream);
int hrseg_copy(const float* in, int ldin, float* out, int ldout, int accumulate, long npix, int C,
               hrseg_stream_t stream);
int hrseg_relu_bwd(const float* dz, int lddz, const float* z, int ldz, float* dx, int lddx,
                   long npix, int C, hrseg_stream_t stream);
int hrseg_nchw_to_nhwc(const float* in, float* out, int ldout, int B, int C, int H, int W,
                       hrseg_stream_t stream);
int hrseg_nhwc_to_nchw(const float* in, int ldin, float* out, int B, int C, int H, int W,
                       hrseg_stream_t stream);

/* ------------------------------------------------------------------ FiLM + heads (csrc/head.hip)
 * FiLM (models.py:58-77), outconv / classifier 1x1 heads (:180,:626-645) and the
 * resize of their logits; the fused head backward hrseg_head_bn_bwd_* is in csrc/bn.hip. */
/* cond[b,c] = mean_{h,w} P[b,c,h,w]  (NCHW in); scratch: BC*64 doubles */
int hrseg_gap_nchw(const float* p, float* cond, double* scratch, int BC, long hw,
                   hrseg_stream_t stream);
/* gb[b, 0:2F] = cond[b,:] @ Wl^T + bl   (Wl: [2F][Cc]) */
int hrseg_film_linear_fwd(const float* cond, const float* wl, const float* bl, float* gb, int B,
                          int Cc, int F2, hrseg_stream_t stream);
/* dcond = dcond_scale * dgb @ Wl (written); dWl += dgb^T cond; dbl += sum_b dgb */
int hrseg_film_linear_bwd(const float* cond, const float* wl, const float* dgb, float* dcond,
                          float* dwl, float* dbl, int B, int Cc, int F2, float dcond_scale,
                          hrseg_stream_t stream);
/* head: z[b,pix,c] = sum_k W[c][k]*(f[b,pix,k]*gamma[b,k]+beta[b,k]) + bias[c];
 * gb = [B][2F] (gamma | beta) or NULL for no FiLM; z is NHWC with row stride
 * ldz; Cout <= 8. */
int hrseg_head_fwd(const float* f, int ldf, const float* gb, const float* w, const float* bias,
                   float* z, int ldz, int B, long hw, int F, int Cout, hrseg_stream_t stream);
/* backward of the head: df (=|+=) gamma*(W^T dz) (df may be NULL); dW, dbias +=
 * (atomics); dgb[b] += (sum_pix f*(W^T dz) | sum_pix W^T dz) when gb != NULL */
int hrseg_head_bwd(const float* f, int ldf, const float* gb, const float* w, const float* dz,
                   int lddz, float* df, int lddf, int df_accumulate, float* dw, float* dbias,
                   float* dgb, int B, long hw, int F, int Cout, hrseg_stream_t stream);
/* The level heads on the UN-NORMALISED output of the layer in front of them (the HRNet shared head, models.py:614): where a
 * conv + BatchNorm + ReLU output z = max(y * scale + shift, 0) has no residual and the level heads are its only readers,
 * neither z nor its gradient has to exist in memory.  hrseg_head_bn_fwd is hrseg_head_fwd reading y (row stride ldy) and the
 * BatchNorm's coef ([mean, rstd, scale, shift][F], hrseg_bn_fwd_t.coef after the finalize phase); it evaluates the expression
 * of the BatchNorm apply phase on load, so the logits are the bits hrseg_bn_fwd_group + hrseg_head_fwd give. */
int hrseg_head_bn_fwd(const float* y, int ldy, const float* coef, const float* gb, const float* w, const float* bias,
                      float* z, int ldz, int B, long hw, int F, int Cout, hrseg_stream_t stream);
/* Backward of the same region in two passes over y.  y holds nseg (1..8) equal segments of B samples of hw pixels (the
 * batched level passes); segment s has its own head: w[s] [Cout[s]][F], FiLM pair gb[s] [B][2F] or NULL, logit gradient
 * dzl[s] [B*hw][lddzl[s]].  With f = max(y * scale + shift, 0), u = sum_c W[c][:] dzl[pix][c] and g = (f > 0) ? gamma * u : 0:
 *   hrseg_head_bn_bwd_reduce, segments [seg0, seg0 + nsegs): what hrseg_head_bwd accumulates (dw[s], dbias[s] +=, dgb[s] +=
 *     when gb[s] != NULL; atomics, not offered in deterministic mode: HRSEG_ERR_UNSUPPORTED) AND the BatchNorm backward's
 *     partial sums of g and g * xhat in the layout and summation order of hrseg_bn_bwd_group's reduce phase with nseg
 *     segments (chunks [s * nchunks / nseg, (s + 1) * nchunks / nseg) belong to segment s); resets dy_absmax.  A level whose
 *     logit gradient depends on another level's dgb (FiLM) is launched after it: one call per level, or one for all.
 *   then hrseg_bn_bwd_group_phases(..., phases 2) on the same partial / nchunks / nseg: totals, dgamma, dbeta (unchanged).
 *   hrseg_head_bn_bwd_apply, all segments: recomputes g and writes dy = scale * (g - mean g - xhat * mean g xhat), raising
 *     dy_absmax as hrseg_bn_bwd_group's apply phase does.
 * The zero fill of the feature gradient, hrseg_head_bwd's write of it and the two reads of it by the BatchNorm backward
 * are gone.  partial: (nchunks + nseg) * 2 * F doubles; nchunks a multiple of nseg. */
#define HRSEG_HEAD_BN_MAX_SEG 8
typedef struct {
  const float* y; int ldy; const float* coef;
  int F, nseg, B; long hw;
  double* partial; int nchunks;
  float* dy_absmax;                                  /* optional, 64 floats, as hrseg_bn_bwd_t.dy_absmax */
  float* dy; int lddy;                               /* out of the apply pass: [nseg*B*hw][F]            */
  const float* gb[HRSEG_HEAD_BN_MAX_SEG]; const float* w[HRSEG_HEAD_BN_MAX_SEG];
  const float* dzl[HRSEG_HEAD_BN_MAX_SEG]; int lddzl[HRSEG_HEAD_BN_MAX_SEG]; int Cout[HRSEG_HEAD_BN_MAX_SEG];
  float* dw[HRSEG_HEAD_BN_MAX_SEG]; float* dbias[HRSEG_HEAD_BN_MAX_SEG]; float* dgb[HRSEG_HEAD_BN_MAX_SEG];
} hrseg_head_bn_t;
int hrseg_head_bn_bwd_reduce(const hrseg_head_bn_t* p, int seg0, int nsegs, hrseg_stream_t stream);
int hrseg_head_bn_bwd_apply(const hrseg_head_bn_t* p, hrseg_stream_t stream);
/* logits resize: NHWC low-res [B,Hi,Wi,C<=16] -> NCHW [B,C,Ho,Wo] bilinear
 * (F.interpolate at models.py:757,766,776) and its transpose */
int hrseg_logits_up_fwd(const float* in, int ldin, int B, int Hi, int Wi, int C, float* out, int Ho,
                        int Wo, int align_corners, hrseg_stream_t stream);
int hrseg_logits_up_bwd(const float* dout, int B, int Hi, int Wi, int C, float* din, int lddin,
                        int Ho, int Wo, int align_corners, hrseg_stream_t stream);

/* ------------------------------------------------------------------ composition over the class tree (csrc/compose.hip)
 * sigmoid / grouped-softmax probability composition (models.py:266-304,:763-798),
 * consistency (Metrics/losses.py:150-177) and the opt-in grouped KL (:180-210):
 * the entry points that take the tree's group table.                         */
/* P0 = sigmoid(z0) ; NCHW */
int hrseg_sigmoid_fwd(const float* z, float* p, long n, hrseg_stream_t stream);
/* level L>0: groups given as parent channel index + child count per group
 * (group_parent / group_size are HOST arrays, copied into the launch) */
int hrseg_compose_fwd(const float* z, const float* pprev, float* p, int B, int C, int Cprev,
                      long hw, int ngroups, const int* group_parent, const int* group_size,
                      hrseg_stream_t stream);
/* backward through composition: inputs dP (strided: element (b,c,i) at
 * b*sb + c*sc + i*si, so a broadcast GAP gradient needs no materialisation),
 * outputs dz (NCHW, accumulate flag) and dPprev (NCHW, accumulate flag). */
int hrseg_compose_bwd(const float* dp, long sb, long sc, long si, const float* z,
                      const float* pprev, float* dz, int dz_accumulate, float* dpprev,
                      int dpprev_accumulate, int B, int C, int Cprev, long hw, int ngroups,
                      const int* group_parent, const int* group_size, hrseg_stream_t stream);
int hrseg_sigmoid_bwd(const float* dp, long sb, long sc, long si, const float* z, float* dz,
                      int accumulate, int B, int C, long hw, hrseg_stream_t stream);
/* sum |sum_{c in group} P[b,c] - Pprev[b,parent]| per group -> out[ngroups] (double, +=) */
int hrseg_consistency(const float* p, const float* pprev, double* out, int B, int C, int Cprev,
                      long hw, int ngroups, const int* group_parent, const int* group_size,
                      hrseg_stream_t stream);
/* gradient of  scale * sum_groups sum_{b,pix} |...|  times the device scalar g[0]:
 * dp [B,C,hw] and dpprev [B,Cprev,hw] are written */
int hrseg_consistency_bwd(const float* p, const float* pprev, const float* g, float scale, float* dp,
                          float* dpprev, int B, int C, int Cprev, long hw, int ngroups,
                          const int* group_parent, const int* group_size, hrseg_stream_t stream);
/* Grouped conditional KL, the opt-in stabiliser the reference keeps commented out (Metrics/losses.py:180-210): per parent
 * group of the level Q = softmax_c(z_c + log(Pprev[parent] + 1e-6)).clamp_min(1e-8) over the group's children;
 * out[g] (double, +=) = sum over b, pixels and the group's children of Q * (log Q + log size_g), i.e. KL(Q || Uniform)
 * before the mean.  hrseg_group_kl_bwd writes dz [B,C,hw] = g[0] * scale * d/dz sum_g out[g] / size_g (Pprev gets no
 * gradient: the log-bias is constant inside a group).  Default off in the train loop. */
int hrseg_group_kl(const float* z, const float* pprev, double* out, int B, int C, int Cprev, long hw, int ngroups,
                   const int* group_parent, const int* group_size, hrseg_stream_t stream);
int hrseg_group_kl_bwd(const float* z, const float* pprev, const float* g, float scale, float* dz, int B, int C,
                       int Cprev, long hw, int ngroups, const int* group_parent, const int* group_size,
                       hrseg_stream_t stream);

/* ------------------------------------------------------------------ loss + metrics (csrc/loss.hip)
 * CrossEntropyLoss / SoftDiceLoss (Metrics/losses.py:16-134), prediction prep +
 * confusion counts (train.py:206-231, Metrics/performance_metrics.py:27-141). */
/* partial[b][c][5] += {n, sum t*logp, sum p*t, sum p, sum t} over t!=-1 (double) */
int hrseg_loss_partials(const float* z, const float* t, double* partial, int B, int C, long hw,
                        hrseg_stream_t stream);
/* out[0]=ce, out[1]=dice, out[2]=dice_valid_count; coef[b][c][4] for the backward */
int hrseg_loss_finalize(const double* partial, const float* w, int B, int C, float* out,
                        float* coef, hrseg_stream_t stream);
/* dz (=|+=) g_ce*dCE/dz + g_dice*dDice/dz ; g = device pointer to {g_ce,g_dice} */
int hrseg_loss_bwd(const float* z, const float* t, const float* coef, const float* g, float* dz,
                   int accumulate, int B, int C, long hw, hrseg_stream_t stream);
/* The same three with the loss options, by value (the entry points above are these at gamma = 0, smooth = 0, alpha = beta =
 * 0.5, bit for bit).  Valid pixels t != -1, w the class weights, I = sum_c w_c sum p t, P = sum_c w_c sum p, T = sum_c w_c sum t:
 *   gamma  focal exponent of the CE: the per-pixel term is -t (1-p)^gamma log p, with 1 - p_c taken as the other channels'
 *          share of the softmax sum (never as a subtraction, which is 0 in fp32 at saturated pixels); 0 in the limit 1-p -> 0.
 *          partials and bwd must be given the same gamma.
 *   smooth, alpha, beta  Dice item = 1 - (2I + smooth) / (2(1-alpha-beta) I + 2 alpha P + 2 beta T + smooth): Tversky weights
 *          alpha on the false positives P - I and beta on the false negatives T - I; an item is valid (counted in out[2], part
 *          of the mean) iff its denominator is not 0, so smooth > 0 keeps every item.
 * Each option must be finite and >= 0: anything else is refused (-1, the message starts with the entry point's name) before a
 * launch.  A NaN logit gives a NaN CE and a NaN dz at its pixel under every option. */
int hrseg_loss_partials_opt(const float* z, const float* t, double* partial, int B, int C, long hw,
                            float gamma, hrseg_stream_t stream);
int hrseg_loss_finalize_opt(const double* partial, const float* w, int B, int C, float smooth, float alpha,
                            float beta, float* out, float* coef, hrseg_stream_t stream);
int hrseg_loss_bwd_opt(const float* z, const float* t, const float* coef, const float* g, float* dz,
                       int accumulate, int B, int C, long hw, float gamma, hrseg_stream_t stream);
/* Online hard example mining for the CE term (csrc/loss_ohem.hip), per level, over the level's whole batch.
 * With p = softmax(z) over all C channels, a pixel is a CANDIDATE iff some channel has t != -1; its score is
 * q = sum over those channels of t_c p_c (non-candidates: -1).  N = number of candidates; lam_k = the min(min_kept, N)-th
 * smallest candidate score when min_kept >= 1 and N >= 1, else -1 (NaN scores sort last).  A candidate is KEPT iff
 * q is NaN, q < thresh, or q <= lam_k: ties at lam_k are all kept, so n_kept >= min(min_kept, N), and a NaN logit stays loud.
 *   hrseg_ohem_scores   one pass over (z, t) writes q[B*hw].
 *   hrseg_ohem_select   q[n] -> record (DEVICE, 16 bytes: {float lam_k; int n_candidates; int n_kept; int reserved}), exactly: a
 *                       radix select over the scores' bit patterns with integer counts, no sort, no host read; the same
 *                       input gives the same record whatever the block order.  `workspace` (DEVICE, 4-byte aligned,
 *                       hrseg_ohem_workspace_bytes() bytes) is zeroed by the call's own first launch.  7 launches.
 *   hrseg_loss_partials_ohem / hrseg_loss_bwd_ohem   hrseg_loss_partials_opt / hrseg_loss_bwd_opt with the CE slots of
 *                       partial (n and sum t (1-p)^gamma log p) and the CE part of dz restricted to kept pixels; both take
 *                       the decision from the stored q and the record, never from a recomputed score.  The Dice slots and
 *                       the Dice part of dz are those of the plain calls.  hrseg_loss_finalize[_opt] runs between them
 *                       unchanged: an item with a class mask that is empty AFTER the selection is the constant 1.0.
 * The selection is a constant of the step: no gradient flows through q or lam_k.  Refused (-1, the message starts with the
 * entry point's name) before any launch: null pointers, thresh outside [0, 1] or not finite, min_kept < 0, n <= 0 or beyond
 * 2^31 - 1, C outside 1..16.  Every launch of these four is counted under the family "ohem" (outside the NULL total). */
size_t hrseg_ohem_workspace_bytes(void);
int hrseg_ohem_scores(const float* z, const float* t, float* q, int B, int C, long hw, hrseg_stream_t stream);
int hrseg_ohem_select(const float* q, long n, float thresh, long min_kept, void* workspace, void* record,
                      hrseg_stream_t stream);
int hrseg_loss_partials_ohem(const float* z, const float* t, const float* q, const void* record, float thresh,
                             double* partial, int B, int C, long hw, float gamma, hrseg_stream_t stream);
int hrseg_loss_bwd_ohem(const float* z, const float* t, const float* q, const void* record, float thresh,
                        const float* coef, const float* g, float* dz, int accumulate, int B, int C, long hw,
                        float gamma, hrseg_stream_t stream);
/* ---- border weights (csrc/border_weight.hip, csrc/loss.hip; Metrics/border.py)
 * The U-Net weight map w(x) = 1 + w0 exp(-d(x)^2 / (2 sigma^2)), d = the distance to the nearest border of the level's label
 * map, computed on the device per step and per level, and the per-pixel weight on the CE term that consumes it.
 *
 * Weight map of one level.  Input t [B,C,H,W] fp32, the level's target planes as hrseg_encode_targets / the partial-label
 * rules write them (-1 / 0 / 1), 1 <= C <= 16.
 *   on_c(i)   iff t[b,c,i] == 1.0f.
 *   void(i)   iff every channel is -1.0f (the loss gives such a pixel a gradient of exactly 0 at this level).
 *   label(i)  the smallest c with on_c(i), or C when no channel is on; any other value (0, NaN, 0.5, ...) is "not on, not -1".
 *             The label byte written to `labels` is label(i) (0..C), or 255 for a void pixel.
 *   d2(i)     for a non-void pixel the minimum of dx^2 + dy^2 over the pixels j of the same image that are not void, have
 *             label(j) != label(i) and dx^2 + dy^2 <= radius^2; 0 when there is no such j, and for void pixels.  Void pixels
 *             are never a source: an ignored region or an unlabelled corner makes no border, and a different label behind a
 *             void gap still counts.  Images do not see each other, and nothing exists outside the frame.
 *   v(i)      lut[d2(i)].  lut is a DEVICE table of radius^2 + 1 floats built on the host: lut[0] = 1.0f,
 *             lut[k] = (float)(1 + w0 exp(-k / (2 sigma^2))) evaluated in fp64.
 * Everything up to the table lookup is integer arithmetic: labels, d2 and v are exact, the same bytes in every run and equal
 * bit for bit to a host reference that uses the same table.
 *   hrseg_border_weights   labels (B*H*W bytes) and v (B*H*W floats) are required outputs, d2 (B*H*W ints) may be NULL.  Two
 *             launches (label extraction, then the search from LDS tiles of hrseg_border_tile pixels plus a radius-wide halo),
 *             no host read, no synchronisation; counted under the family "border_weights" (outside the NULL total).  Refused
 *             (-1, the message starts with the entry point's name) before any launch: a null t, lut, labels or v, B < 1,
 *             C outside 1..16, H < 1 or W < 1, H*W >= 2^31, radius outside 1..32.
 *
 * Per-pixel weights in the fused loss.  pw [B*hw] fp32 holds one weight per pixel and applies to the CE term only (as the
 * OHEM selection does):
 *   hrseg_loss_partials_pw   hrseg_loss_partials_opt with slots 0 and 1 of partial[b][c][5] = sum pw and
 *             sum pw t (1-p)^gamma log p over t != -1; slots 2..4 are those of the plain call.  hrseg_loss_finalize[_opt]
 *             runs unchanged behind it, so the CE of a class mask is the pw-weighted mean, a mask whose weighted mass is <= 0
 *             counts as empty (the item is the constant 1.0) and a constant map gives the loss of the unweighted call.
 *   hrseg_loss_bwd_pw        hrseg_loss_bwd_opt with the CE part of dz at a pixel multiplied by pw there; the Dice part is
 *             untouched.
 * pw finite and >= 0 is the caller's duty; no gradient flows to pw.  A NaN logit gives a NaN CE and a NaN dz at its pixel
 * whatever its weight (0 * NaN stays NaN).  Not combined with OHEM.  The refusals of the _opt entry points apply, plus a null
 * pw, each under the _pw entry point's name; the launches are counted like those of the plain loss calls (not at all). */
#define HRSEG_BORDER_TILE_W 64
#define HRSEG_BORDER_TILE_H 16
#define HRSEG_BORDER_MAX_RADIUS 32
int hrseg_border_tile(int* w, int* h);    /* the tile of the search kernel, for tests (as hrseg_components_tile) */
int hrseg_border_weights(const float* t, int B, int C, int H, int W, int radius, const float* lut,
                         unsigned char* labels, float* v, int* d2, hrseg_stream_t stream);
int hrseg_loss_partials_pw(const float* z, const float* t, const float* pw, double* partial, int B, int C, long hw,
                           float gamma, hrseg_stream_t stream);
int hrseg_loss_bwd_pw(const float* z, const float* t, const float* pw, const float* coef, const float* g, float* dz,
                      int accumulate, int B, int C, long hw, float gamma, hrseg_stream_t stream);
/* ---- tree distillation (csrc/distill.hip; Metrics/losses.py TreeDistillation)
 * A loss that pulls the student's distribution towards a teacher's, level by level: per sibling group the KL between the
 * teacher's and the student's conditional distribution over the children, weighted by the teacher's composed probability of
 * the parent (the soft form of the restrictive -1 mask).  With those weights the sum over the levels is the KL between the two
 * composed leaf distributions (chain rule of KL).
 *
 * One level.  z [B,C,hw] fp32 NCHW the student logits, u the teacher logits of the same shape, wprev [B,Cprev,hw] the teacher's
 * parent probabilities or NULL (every weight is 1; the parents of the group table are not read and Cprev is ignored), pw [B*hw]
 * one weight per pixel or NULL (1).  The group table is that of hrseg_compose_fwd: consecutive groups, sizes sum to C, C <= 16;
 * level 0 and flat models pass one group of size C with wprev = NULL.  inv_temp = beta = 1/T, finite and > 0; thresh in [0, 1].
 * Per pixel i of image b and group g with channels c, everything in fp32, no operation fused with another:
 *   a_c = beta * u_c,  ma = max_c a_c,  xa_c = a_c - ma,  lq_c = xa_c - log(sum_c exp(xa_c)),  q_c = exp(xa_c) * (1 / sum_c exp(xa_c))
 *   lp_c, p_c         the same from z
 *   kl_g = sum_c q_c * (lq_c - lp_c)       a saturated q_c = 0 gives 0 * finite = 0, never 0 * log 0; a group of one gives
 *                                          exactly 0 and a gradient of exactly 0; u == z gives exactly 0 and 0
 *   omega_g = wprev[b, parent_g, i] or 1;  m = pw[b*hw + i] or 1
 *   conf_g = omega_g / sum_c exp(u_c - max_c u_c)      the teacher's composed probability of the group's top child at
 *                                          temperature 1 whatever beta is: with wprev the model's own composition, the hedged
 *                                          decode's T_L of a path through this group
 *   the group is DROPPED iff conf_g < thresh (fp32, <): a NaN conf is never dropped, and thresh = 0 keeps everything and gives
 *   the bits of the instance without the gate.
 *   hrseg_tree_kl       out[g][3] (double, +=) = the sums over the kept (pixel, group) pairs of (m * omega_g) * kl_g and of
 *             m * omega_g, and their number.  Per-thread and per-block sums are fp64; one atomicAdd per block and slot, and under
 *             the `deterministic` knob one block in all, so two runs give the same bytes.
 *   hrseg_tree_kl_bwd   dz[b,j,i] (=|+=, `accumulate`) ((g[0] * scale) * (m * omega_g)) * beta * (p_j - q_j) for j in a kept group;
 *             a dropped group writes exactly 0, or adds nothing when accumulating.  g is a DEVICE scalar, scale comes by value.
 *             u, wprev and pw get no gradient.  Both calls must be given the same inv_temp and thresh.
 * Non-finite values.  A NaN among the logits of a kept group, on either side, makes the group's first out slot NaN and dz NaN on
 * the group's channels at that pixel, whatever m and omega_g are (0 * NaN stays NaN); other pixels and groups are untouched.  A
 * teacher NaN makes conf_g NaN, so its group is always kept; a student NaN in a group that the gate drops is dropped with it.
 * Infinite logits, in a group that holds at least one finite logit on that side: a +Inf logit on either side is Inf - Inf = NaN in
 * xa (resp. the student's), so the first out slot and dz on the group's channels are NaN as for a NaN; conf_g is NaN too (kept).
 * A -Inf teacher logit has q_c = 0 and lq_c = -Inf: the first out slot is NaN (0 * -Inf), dz stays finite (q_j = 0 there).  A
 * -Inf student logit has lp_c = -Inf: the first out slot is +Inf where q_c > 0 (NaN where q_c == 0), dz stays finite (p_j = 0).
 * One launch per call, no workspace, no allocation, no synchronisation; counted under the family "tree_kl" (outside the NULL
 * total).  Refused (-1, the message starts with the entry point's name) before any launch: a null z, u, out, g or dz, B < 1,
 * C outside 1..16, hw < 1, a bad group table (the three messages of hrseg_compose_fwd's), wprev set with Cprev outside 1..16 or
 * a parent outside Cprev, inv_temp not finite or <= 0, thresh outside [0, 1] or NaN. */
int hrseg_tree_kl(const float* z, const float* u, const float* wprev, const float* pw, float inv_temp, float thresh,
                  double* out, int B, int C, int Cprev, long hw, int ngroups, const int* group_parent,
                  const int* group_size, hrseg_stream_t stream);
int hrseg_tree_kl_bwd(const float* z, const float* u, const float* wprev, const float* pw, float inv_temp, float thresh,
                      const float* g, float scale, float* dz, int accumulate, int B, int C, int Cprev, long hw,
                      int ngroups, const int* group_parent, const int* group_size, hrseg_stream_t stream);
/* per-class metric vectors of nlevels (1..8) levels from their confusion counts in ONE launch: cm[L] (DEVICE, int64
 * [K_L][K_L], (target, predicted) as hrseg_predict_metrics counts them), child[L] != 0: label 0 is the synthetic background
 * of a child level (its row is dropped, its class not reported).  out (DEVICE) receives [5][sum_L (K_L - child_L)] floats:
 * accuracy (= recall per class, as the reference defines it), iou, dice, precision, recall, levels side by side; a zero
 * denominator gives 0.  Replaces the ~80 small tensor ops of the reference's metric classes per batch (train.py:47-51,
 * Metrics/performance_metrics.py).  cm, K, child are HOST arrays. */
int hrseg_metric_vectors(int nlevels, const long long* const* cm, const int* K, const int* child, float* out,
                         hrseg_stream_t stream);
/* argmax one-hot of z masked by t!=-1, plus confusion matrix counts
 * cm[(C+child)*(C+child)] (int64, +=) of (target label, predicted label) with
 * the synthetic background class 0 for child levels. mask_pred=1 is the train
 * loop (predictions/targets zeroed where t==-1), 0 the test loop (z holds
 * probabilities, raw targets). onehot may be NULL. */
int hrseg_predict_metrics(const float* z, const float* t, float* onehot, long long* cm, int B,
                          int C, long hw, int child, int mask_pred, hrseg_stream_t stream);

/* ------------------------------------------------------------------ optimizer
 * torch.optim.AdamW (train.py:513-516) over one flat fp32 parameter buffer. */
int hrseg_adamw(float* p, const float* g, float* m, float* v, long n, float lr, float beta1,
                float beta2, float eps, float weight_decay, float bc1, float bc2, float gscale,
                hrseg_stream_t stream);
/* same update with every scalar in DEVICE memory (hipGraph-replayable): hyper = {lr, beta1, beta2,
 * eps, weight_decay, grad_scale}; state = {step, 1-beta1^step, 1/sqrt(1-beta2^step)} is advanced by
 * one step per call. */
int hrseg_adamw_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper,
                    float* state, hrseg_stream_t stream);
int hrseg_fill(float* p, float v, long n, hrseg_stream_t stream);

/* ------------------------------------------------------------------ gradient clipping / non-finite step skip
 * Global L2 norm of the flat gradient buffer AdamW is about to consume, torch.nn.utils.clip_grad_norm_'s
 * coefficient from it, and an AdamW step that applies the coefficient or leaves everything alone when a gradient
 * element is not finite.  With g the buffer and s = hyper[5] (grad_scale):
 *   S = sum (double)g_i * (double)g_i   (fp64 from the first multiply on: no fp32 overflow or underflow)
 *   norm = |s| * sqrt(S);  finite = isfinite(S) && isfinite(s);  coef = min(1, max_norm / (norm + 1e-6))
 * evaluated in fp64 and stored as fp32.  max_norm = +inf gives coef == 1.0f exactly.
 * The sum is taken over hrseg_grad_sumsq_chunks(n) chunks of hrseg_grad_sumsq_chunk_len() floats, one fp64 partial each;
 * chunking and summation order depend on n alone, no atomics: bit-reproducible, and equal on every rank that holds
 * the same bytes.  A launch uses at most hrseg_grad_sumsq_max_blocks() blocks (more chunks: a block takes several).
 * Device buffers: clipcfg = {max_norm, skip_nonfinite (0 or 1)}; clip = {norm, coef, finite (0 or 1), skipped_total};
 * partial = nchunks doubles.  hrseg_grad_clip_finalize also advances state = {step, 1-beta1^step,
 * 1/sqrt(1-beta2^step)} by one step (what hrseg_adamw_dev does itself) -- unless skip_nonfinite is set and finite is 0:
 * then the step is void, state stays, skipped_total goes up by one, and hrseg_adamw_dev_clip returns without touching
 * p, m, v.  Otherwise hrseg_adamw_dev_clip is hrseg_adamw_dev's update with the gradient (g * s) * coef; with
 * coef == 1 it is bit-identical to it.  Order per step: hrseg_grad_sumsq, hrseg_grad_clip_finalize,
 * hrseg_adamw_dev_clip, on one stream. */
int hrseg_grad_sumsq_chunk_len(void);
int hrseg_grad_sumsq_max_blocks(void);
int hrseg_grad_sumsq_chunks(long n);                    /* number of partials for n elements; -1: n out of range */
int hrseg_grad_sumsq(const float* g, long n, double* partial, int nchunks, hrseg_stream_t stream);
int hrseg_grad_clip_finalize(const double* partial, int nchunks, const float* hyper, const float* clipcfg,
                             float* state, float* clip, hrseg_stream_t stream);
int hrseg_adamw_dev_clip(float* p, const float* g, float* m, float* v, long n, const float* hyper,
                         const float* state, const float* clipcfg, const float* clip, hrseg_stream_t stream);

/* ------------------------------------------------------------------ weight EMA (exponential moving average)
 * A shadow e[n] of the flat parameter buffer, advanced once per optimizer step in fp32:
 *   t = s - s0 - 1;  eff = warmup ? min(d, (1 + t) / (10 + t)) : d;  alpha = 1 - eff;  e = e + (p' - e) * alpha
 * p' = the parameter AFTER this step's AdamW update, s = state[0] after this step's tick, and the device buffer
 * emacfg = {d = decay, warmup (0 or 1), s0 = the value of state[0] when averaging began}: t counts the updates already
 * done, taken from AdamW's own step counter (a void step advances neither).  The product and the sum are one fused
 * multiply-add, fma(p' - e, alpha, e), in every kernel below, so they agree bit for bit.
 * hrseg_adamw_dev_ema is hrseg_adamw_dev (state advanced by one step) and hrseg_adamw_dev_clip_ema is hrseg_adamw_dev_clip
 * (state advanced by hrseg_grad_clip_finalize; a void step leaves e untouched as well) with the line above appended per
 * element: p, m, v come out bit-identical to those entry points, e costs one more 16-byte load and store per four
 * elements and no launch.  hrseg_ema_update is the line alone, for a p that has its step behind it.  hrseg_swap
 * exchanges the contents of two flat fp32 buffers that do not overlap (the shadow and the parameters: addresses held
 * elsewhere stay valid).  Every buffer 16-byte aligned; e a buffer of its own. */
int hrseg_adamw_dev_ema(float* p, const float* g, float* m, float* v, float* e, long n, const float* hyper,
                        float* state, const float* emacfg, hrseg_stream_t stream);
int hrseg_adamw_dev_clip_ema(float* p, const float* g, float* m, float* v, float* e, long n, const float* hyper,
                             const float* state, const float* clipcfg, const float* clip, const float* emacfg,
                             hrseg_stream_t stream);
int hrseg_ema_update(float* e, const float* p, long n, const float* state, const float* emacfg,
                     hrseg_stream_t stream);
int hrseg_swap(float* a, float* b, long n, hrseg_stream_t stream);

/* ------------------------------------------------------------------ gradient exchange (data parallelism)
 * Thin wrappers over RCCL for the one collective of the path: the in-place sum of a flat fp32 gradient
 * bucket over the ranks (replaces nn.DataParallel's reduce-add, train.py:509-510).  librccl.so is opened
 * on first use.  One communicator per process (= per GPU); the 128-byte id comes from ONE rank and is
 * shipped to the others by the caller (file, TCP store, ...).  All calls are stream-ordered, none
 * synchronises the host. */
int hrseg_comm_unique_id(void* id128);
int hrseg_comm_init(void** comm, int rank, int world, const void* id128);   /* collective over the ranks */
int hrseg_comm_allreduce_async(void* comm, float* buf, long count, hrseg_stream_t stream);
int hrseg_comm_wait(hrseg_stream_t comm_stream, hrseg_stream_t consumer);   /* consumer waits for comm_stream */
int hrseg_comm_destroy(void* comm);

/* ------------------------------------------------------------------ target encoding (input side of the path; csrc/targets.hip)
 * SegDataset.separate_masks / traverse_tree / process_ignore_values (Data/dataset.py:41-124,
 * 227-265): label image [B,hw] of uint8 pixel values -> out [B,C,hw] fp32 (NCHW planes).
 * on_lut: DEVICE table [256] of uint64, bit c set when channel c's node contains the leaf class
 * with that pixel value; parent: HOST array [C], channel index of the node's direct parent or -1
 * (roots, and every channel in flat mode).  Channel value: 1 on the node, else 0 for roots / inside
 * the parent's area, else -1.  C <= 64. */
int hrseg_encode_targets(const unsigned char* label, const unsigned long long* on_lut, const int* parent,
                         float* out, int B, int C, long hw, hrseg_stream_t stream);

/* ------------------------------------------------------------------ device input pipeline (Data/augment.py)
 * The reference's per-sample transforms (Data/dataloaders.py:49-70, Data/dataset.py:397-470) for a batch of RAGGED
 * uint8 sources: one packed byte buffer plus a DEVICE descriptor table desc [B][4] of int64 (byte offset, H, W,
 * channels 1|3; 3 = interleaved HWC).  Output: x [B,3,S,S] fp32 in [-1,1], y [B,C,S,S] fp32 targets as
 * hrseg_encode_targets.  params: DEVICE table [B][HRSEG_AUG_PARAMS] fp32 drawn on the host, laid out as below.
 * Workspaces: hrseg_augment_workspace gives the bytes each entry point needs (eval mode needs none). */
#define HRSEG_AUG_PARAMS 48
#define HRSEG_AUG_P_FLAGS 0      /* HRSEG_AUG_HFLIP | HRSEG_AUG_VFLIP | HRSEG_AUG_WARP, as a float */
#define HRSEG_AUG_P_ORDER 1      /* [4] ColorJitter order: 0 brightness, 1 contrast, 2 saturation, 3 hue */
#define HRSEG_AUG_P_BRIGHT 5     /* brightness factor b */
#define HRSEG_AUG_P_CONTRAST 6   /* [2] c, (float)(1 - c) */
#define HRSEG_AUG_P_SAT 8        /* [2] s, (float)(1 - s) */
#define HRSEG_AUG_P_HUE 10       /* hue shift */
#define HRSEG_AUG_P_THETA 12     /* [6] torchvision affine theta, transposed and divided by (S/2): t0 t1 / t2 t3 / t4 t5 */
#define HRSEG_AUG_P_TAPS 18      /* [25] normalised 1-D Gaussian blur taps */
#define HRSEG_AUG_HFLIP 1
#define HRSEG_AUG_VFLIP 2
#define HRSEG_AUG_WARP 4
int hrseg_augment_workspace(int B, int S, size_t* image_bytes, size_t* target_bytes);
/* train: resize + 25x25 Gaussian blur + ColorJitter + normalise + flips + nearest affine (fill -1), 2 launches;
 * eval (train == 0): resize + normalise, 1 launch, params and work unused.  S > 12 in train mode. */
int hrseg_augment_image(const unsigned char* src, const long* desc, const float* params, float* x, int B, int S,
                        int train, void* work, size_t work_bytes, hrseg_stream_t stream);
/* per-node masks of the label (on_lut / parent exactly as hrseg_encode_targets), resized with antialias (torch
 * _upsample_bilinear2d_aa) or plain bilinear, thresholded at 0.5 and encoded.  warp: flips + nearest affine with the
 * reference's fill rule (channel 0: max of its resized mask, other channels: -1 before the threshold), 2 launches;
 * warp == 0: 1 launch, params and work unused. */
int hrseg_augment_targets(const unsigned char* label, const long* desc, const unsigned long long* on_lut,
                          const int* parent, const float* params, float* y, int B, int C, int S, int warp,
                          int antialias, void* work, size_t work_bytes, hrseg_stream_t stream);

/* ------------------------------------------------------------------ partial labels (csrc/targets.hip, csrc/augment.hip)
 * Label maps that say less than a leaf per pixel: an IGNORE byte (the pixel takes no part in loss or gradient) and the byte
 * of an INTERNAL node ("tooth", child unknown: the pixel supervises the levels down to that node and nothing below).  This
 * is the one statement of the semantics; everything else refers here.
 *
 * Every byte v has two sets over the emitted channels (all nodes breadth first, or the leaves in flat mode):
 *   leaf byte               on[v] = the leaf and its ancestors             unk[v] = empty
 *   internal byte of node n on[v] = n and its ancestors (where channels)   unk[v] = every channel strictly below n
 *   ignore byte             on[v] = empty                                  unk[v] = every channel
 *   any other byte          on[v] = empty                                  unk[v] = empty
 * Channel c of a pixel with the sets (ON, UNK):
 *   1. 1 if c is in ON;  2. else -1 if c is in UNK;  3. else 0 if c is a root or its direct parent is in ON;  4. else -1.
 * With UNK empty this is the rule of hrseg_encode_targets.  So a "tooth" pixel has tooth and its ancestors 1, their
 * siblings 0, and every channel below tooth -1 (with tooth a root: the other roots 0, everything below level 0 -1); an ignored pixel is -1 in every channel, level 0
 * included; in flat mode an internal byte gives -1 on the leaves below the node and 0 on the others.  The loss kernels mask
 * per channel with t != -1, and a pixel whose channels are all -1 at a level gets a gradient of exactly 0 there.
 *
 * Resized targets accumulate two coverages per channel over the footprint of hrseg_augment_targets, with exactly its
 * weights, order and fp32 arithmetic: cover_on[c] = sum of w where on_c holds, cover_may[c] = sum of w where on_c or unk_c
 * holds.  ON_c = cover_on[c] >= 0.5, MAY_c = cover_may[c] >= 0.5, UNK_c = MAY_c and not ON_c: a channel is called off (0)
 * only where the known-off share of the footprint is the majority; other mixed footprints fall to unknown.  Adding the same
 * non-negative terms in the same order is monotone in fp32, so cover_may >= cover_on and ON is a subset of MAY; with
 * unk_lut all zero the two sums are bit-equal and the output is that of hrseg_augment_targets.  The nearest warp moves both
 * thresholded sets.  Outside the source frame: fill_unknown == 0 is the rule of hrseg_augment_targets (ON = {channel 0} if
 * channel 0 is covered anywhere in the image, else empty; UNK empty), fill_unknown != 0 sets ON empty and UNK to every
 * channel (the corners a rotation brings in are unlabelled).  The image fill is the same either way.
 *
 * on_lut / unk_lut: DEVICE tables [256] of uint64 (bits at or above C are not read); everything else as for the entry
 * points they stand next to.  hrseg_augment_workspace_partial: the warp workspace holds two uint64 per pixel plus the
 * per-block flags.  Launches count under "augment_targets": 1 without the warp, 2 with. */
int hrseg_encode_targets_partial(const unsigned char* label, const unsigned long long* on_lut,
                                 const unsigned long long* unk_lut, const int* parent, float* out, int B, int C, long hw,
                                 hrseg_stream_t stream);
int hrseg_augment_workspace_partial(int B, int S, size_t* target_bytes);
int hrseg_augment_targets_partial(const unsigned char* label, const long* desc, const unsigned long long* on_lut,
                                  const unsigned long long* unk_lut, const int* parent, const float* params, float* y, int B,
                                  int C, int S, int warp, int antialias, int fill_unknown, void* work, size_t work_bytes,
                                  hrseg_stream_t stream);

/* ------------------------------------------------------------------ mixing (Data/mix.py; csrc/mix.hip)
 * ClassMix / CutMix / paste by tree node: lay pixels of a DONOR sample of the batch, labels included, over a recipient.  This
 * is the one statement of the semantics; everything else refers here.
 *
 * Inputs: x [B,3,S,S] fp32 and y [B,C,S,S] fp32 as hrseg_augment_* write them; in general any in [B,K,S,S] fp32.  A target is
 * one ternary column per pixel (hrseg_encode_targets), so a pasted pixel takes the donor's whole column and stays consistent at
 * every level; an ignored pixel (partial labels) is -1 in every channel and is therefore never chosen by a node, an internal
 * "tooth" pixel is pasted with its unknown children.
 *
 * params: DEVICE table [B][HRSEG_MIX_PARAMS] of int32, one row per sample:
 *   HRSEG_MIX_P_FLAGS   HRSEG_MIX_APPLY | HRSEG_MIX_BOX
 *   HRSEG_MIX_P_DONOR   sample index in [0,B) (a row whose donor is outside is treated as not applied)
 *   HRSEG_MIX_P_DX, _DY the donor's content is moved by (dx, dy) whole pixels: output pixel (r, c) looks at donor pixel
 *                       (r - dy, c - dx); a donor pixel outside the frame is never taken; any int32
 *   HRSEG_MIX_P_BOX     [4] r0, c0, r1, c1, half-open, in output coordinates
 *   the rest            reserved, zero
 *
 * Counts: counts[b][c] = the number of pixels of sample b with y[b][c] == 1.0f, exact int32, over the whole unshifted frame,
 * for all C channels.
 *
 * Node choice, for a sample b with APPLY and without BOX, donor d:
 *   P = {c : cand[c] != 0 and counts[d][c] >= min_pixels},  n = |P|,  k = k_of_n[n],
 *   chosen[b] = the k members of P with the smallest prio[b][c].
 * prio: DEVICE [B][C] int32, each row a permutation of 0..C-1 (no ties; equal values would fall back to the channel index).
 * k_of_n: DEVICE [65] int32 built on the host, k_of_n[0] = 0, else min(n, max(1, ceil(share * n))): the device does no float
 * arithmetic for the choice.  cand: HOST [C] int32 of 0/1, passed like `parent` of hrseg_encode_targets.  chosen is written as
 * one uint64 per sample (bit c = channel c), 0 for BOX samples and for samples that are not applied.  counts may be NULL when
 * no applied sample is without BOX; a sample that would need it then chooses nothing.
 *
 * Mask, uint8 [B,S,S] of 0 / 1:  not APPLY: 0;  BOX: 1 where r0 <= r < r1, c0 <= c < c1 and the moved donor pixel is in the
 * frame;  otherwise: 1 where the moved donor pixel is in the frame and some c in chosen[b] has y[d][c][r-dy][c-dx] == 1.0f.
 *
 * Gather: out[b][k][r][c] = mask[b][r][c] ? in[d][k][r-dy][c-dx] : in[b][k][r][c].  The 32 bits are copied, never blended
 * arithmetically: NaN payloads, infinities and -0.0 come through unchanged.  out must not alias in (a donor can itself be a
 * recipient).  A set mask byte is honoured only on an applied sample and where the moved donor pixel is in the frame (always
 * so for the mask of hrseg_mix_masks with the same params).
 *
 * hrseg_mix_counts clears counts itself (an async memset on the stream) and launches once; hrseg_mix_masks and
 * hrseg_mix_gather are one launch each; all count under "mix".  No entry point synchronises or copies to the host.
 * Limits: 1 <= C <= 64, hw < 2^31, B*C*S*S < 2^31 (masks), B*K*S*S < 2^31 (gather), min_pixels >= 1. */
#define HRSEG_MIX_PARAMS 16
#define HRSEG_MIX_P_FLAGS 0
#define HRSEG_MIX_P_DONOR 1
#define HRSEG_MIX_P_DX 2
#define HRSEG_MIX_P_DY 3
#define HRSEG_MIX_P_BOX 4
#define HRSEG_MIX_APPLY 1
#define HRSEG_MIX_BOX 2
int hrseg_mix_counts(const float* y, int* counts, int B, int C, long hw, hrseg_stream_t stream);
int hrseg_mix_masks(const float* y, const int* counts, const int* params, const int* prio, const int* k_of_n,
                    const int* cand, int min_pixels, unsigned char* mask, unsigned long long* chosen,
                    int B, int C, int S, hrseg_stream_t stream);
int hrseg_mix_gather(const float* in, const unsigned char* mask, const int* params, float* out,
                     int B, int K, int S, hrseg_stream_t stream);

/* ------------------------------------------------------------------ device output pipeline (Data/decode.py)
 * The inverse of the input pipeline: per-level logits at network size -> one label map per source image, at the source's
 * own size, in the pixel values of class_map.csv.  z: HOST array of nlevels DEVICE pointers, level L is [B, C[L], S, S]
 * fp32 NCHW, channels in breadth-first tree order (a flat model: one level over the leaves).  For output pixel (y, x) of
 * sample b (H_b x W_b from desc, laid out as for hrseg_augment_*: byte offset, H, W, 1):
 *   1. every logit that is needed is resampled S x S -> H_b x W_b bilinearly (torch align_corners=False, no antialias);
 *   2. c = arg-max over the level-0 channels (lowest index wins ties);
 *   3. while node c has children: c = arg-max over the consecutive channels of ITS child group at the next level only
 *      (the model's composed probability P_parent * softmax_group(z) has the same arg-max: the decoded path is always
 *      consistent with the tree);
 *   4. labels[offset + y * W_b + x] = pixel value of the leaf reached;
 *   5. confidence (optional, same packing in floats): sigmoid(z_0[c_0]) * prod_L softmax_group(z_L)[c_L]; with
 *      root_softmax (flat models) the level-0 factor is softmax over the level instead of the sigmoid.
 * Limits: nlevels <= 8, C[L] <= 16, sum C[L] <= 64, S <= 32768; labels 4-byte and confidence 16-byte aligned.  The tree
 * travels as a kernel argument: no device allocation, no workspace, no synchronisation.  1 launch, counted under the
 * family "decode_labels". */
#define HRSEG_DECODE_MAX_LEVELS 8
#define HRSEG_DECODE_MAX_CHANNELS 16
typedef struct {
  int first_child[HRSEG_DECODE_MAX_LEVELS][HRSEG_DECODE_MAX_CHANNELS]; /* first channel of the child group at level L+1, or -1 */
  int n_children[HRSEG_DECODE_MAX_LEVELS][HRSEG_DECODE_MAX_CHANNELS];  /* 0: a leaf */
  int pixel_val[HRSEG_DECODE_MAX_LEVELS][HRSEG_DECODE_MAX_CHANNELS];   /* leaves: 0..255 */
  int root_softmax;                                                   /* confidence of level 0: 0 sigmoid, 1 softmax */
} hrseg_decode_tree_t;
int hrseg_decode_labels(int nlevels, const float* const* z, const int* C, const hrseg_decode_tree_t* tree,
                        const long* desc, unsigned char* labels, float* confidence, int B, int S,
                        hrseg_stream_t stream);

/* ------------------------------------------------------------------ hedged decode (Data/hedge.py, csrc/decode_hedged.hip)
 * hrseg_decode_hedged: the decode above, but the walk may end at the parent where the child is unsure.  Inputs as for
 * hrseg_decode_labels plus the hedge table and a counter buffer.  Per output pixel:
 *   1. steps 1-3 of hrseg_decode_labels unchanged: the same resampling, the same strict > arg-max, the same group
 *      restriction; c_0, c_1, ... is the decode's path;
 *   2. T_L is the decode's own running confidence after level L: sigmoid(z_0[c_0]) * prod_{l <= L} softmax_group(z_l)[c_l],
 *      the same product in the same order and with the same rounding as the `confidence` output of hrseg_decode_labels
 *      (as csrc/decode.hip spells it);
 *   3. after choosing c_L the test T_L < tau[L][c_L] is made in fp32 with <; a NaN does not stop the walk, so all-zero
 *      thresholds reproduce hrseg_decode_labels exactly, labels and confidence, non-finite values included.
 *        - true at L == 0: the label is reject_val, the confidence T_0, the row "rejected" is counted;
 *        - true at L >= 1: the label is stop_val[L-1][c_{L-1}], the confidence T_{L-1}, node (L-1, c_{L-1}) is counted; the
 *          pixel fetches nothing deeper;
 *        - otherwise, c_L a leaf: the label is its pixel value, the confidence T_L, node (L, c_L) is counted;
 *        - otherwise the walk descends;
 *   4. stops: DEVICE int64 [B][sum C + 2], accumulated with +=: one cell per tree node in breadth-first channel order, then
 *      "rejected", then "nonfinite".  "nonfinite" counts the pixels whose confidence (step 3; counted whether or not it is
 *      stored) is NaN, on top of their node cell, so the node cells plus "rejected" sum to H*W of the sample.  stops may be
 *      NULL.  Everything counted is an integer: the same bytes in every run and under the "deterministic" knob.
 * Refused, each with a message before anything is launched: every limit and alignment rule of hrseg_decode_labels;
 * tree->root_softmax set (a flat model has no path to shorten); a tau outside [0, 1] or NaN; a stop_val of an internal node
 * outside 0..255; reject_val outside -1..255, or -1 together with a non-zero level-0 tau; any two of {leaf values, internal
 * stop_vals, reject_val} equal; stops not 8-byte aligned.  The sizes live in the device descriptor table, so H*W > 2^31 of a
 * sample is refused by the host wrapper (ops.decode_hedged), as the scorers do it; the kernel leaves such a sample untouched
 * (its 32-bit block counters could wrap).  Entries of tau and stop_val beyond the tree's channels are not read.
 * 1 launch, family "decode_hedged" (never "decode_labels"), outside the NULL total; the tree, the thresholds and the stop
 * values travel as kernel arguments: no workspace, no device allocation, no synchronisation. */
typedef struct {
  float tau[HRSEG_DECODE_MAX_LEVELS][HRSEG_DECODE_MAX_CHANNELS];      /* entering node (L, c) needs T_L >= tau[L][c]; 0 never stops */
  int   stop_val[HRSEG_DECODE_MAX_LEVELS][HRSEG_DECODE_MAX_CHANNELS]; /* internal nodes: the byte written when the walk ends ON that node */
  int   reject_val;                                                   /* byte written where level 0 itself fails; -1: no rejection (then every tau[0][c] must be 0) */
} hrseg_hedge_t;
int hrseg_decode_hedged(int nlevels, const float* const* z, const int* C, const hrseg_decode_tree_t* tree,
                        const hrseg_hedge_t* hedge, const long* desc, unsigned char* labels, float* confidence,
                        long long* stops, int B, int S, hrseg_stream_t stream);

/* ------------------------------------------------------------------ test-time augmentation (predictEval.TestTimeAugment)
 * hrseg_decode_views: the decode above on the MEAN logit of an ensemble of views.  A view v is one set of per-level logits
 * z_v[L] of shape [B, C[L], S_v, S_v] (fp32 NCHW) plus flags f_v in {0, HRSEG_VIEW_HFLIP, HRSEG_VIEW_VFLIP, both}: the
 * network saw the image mirrored along x and/or y (and resized to S_v).  S and flags are HOST arrays of nviews entries, z a
 * HOST array of nviews * nlevels DEVICE pointers, view-major (z[v * nlevels + L]).  For output pixel (y, x) of sample b
 * (H_b x W_b from desc):
 *   1. per view, the row and column taps and weights follow from the output coordinate exactly as in hrseg_decode_labels
 *      (scale S_v / H_b, torch align_corners=False); on a flipped axis the kernel reads source index S_v - 1 - i where it
 *      would have read i, with the same weights: torch.flip of the view's logits followed by F.interpolate(bilinear,
 *      align_corners=False).  The 2 x 2 blend rounds exactly as hrseg_decode_labels rounds it (the same multiplies and
 *      fused multiply-adds in the same order): r_v;
 *   2. mean logit m = ((r_0 + r_1) + ... + r_{V-1}) * (1.0f / V): fp32 round-to-nearest adds in view order, one multiply,
 *      no contraction; with V = 1 this is r_0 bit for bit, and the call returns what hrseg_decode_labels returns;
 *   3. steps 2-5 of hrseg_decode_labels unchanged on m: arg-max over level 0, top-down through the child group of the
 *      chosen node only, leaf pixel value, optional confidence sigmoid(m_0[c_0]) * prod_L softmax_group(m_L)[c_L]
 *      (root_softmax as there).
 * In probability terms a group's soft-max of the mean logit is the normalised geometric mean of the views' group
 * soft-maxes; the decoded path is still always a path of the tree.
 * Limits: 1 <= nviews <= HRSEG_DECODE_MAX_VIEWS, flags[v] in 0..3, 1 <= S[v] <= 32768, and every limit and alignment rule
 * of hrseg_decode_labels; each violation is refused with a message before anything is launched.  Only the groups on the
 * decoded path are fetched (V x 4 taps per channel).  1 launch, counted under the family "decode_views" (never under
 * "decode_labels"), outside the NULL total; no workspace, no device allocation, no synchronisation. */
#define HRSEG_DECODE_MAX_VIEWS 8
#define HRSEG_VIEW_HFLIP 1
#define HRSEG_VIEW_VFLIP 2
int hrseg_decode_views(int nviews, const int* S, const int* flags, int nlevels, const float* const* z, const int* C,
                       const hrseg_decode_tree_t* tree, const long* desc, unsigned char* labels, float* confidence,
                       int B, hrseg_stream_t stream);
/* The network inputs of all flip views of one scale: out [nviews * B, C, H, W], block v is x [B, C, H, W] mirrored as
 * flags[v] says (HOST array; 0: a plain copy).  An exact copy of bits, float4 moves where W % 4 == 0 and both tensors are
 * 16-byte aligned.  The blocks then go through ONE eval-mode forward of batch nviews * B (eval-mode BatchNorm uses the
 * running statistics: samples do not interact).  nviews <= HRSEG_DECODE_MAX_VIEWS, fewer than 2^31 output elements.
 * 1 launch, family "flip_views", outside the NULL total. */
int hrseg_flip_views(const float* x, float* out, int nviews, const int* flags, int B, int C, int H, int W,
                     hrseg_stream_t stream);

/* ------------------------------------------------------------------ sliding-window inference (predictEval.SlidingWindow)
 * The network runs on overlapping S x S windows of a CANVAS of each image and the windows' logits are blended where they
 * overlap.  The canvas Hc x Wc (Hc, Wc >= S) exists as arithmetic only: no canvas-size tensor is ever allocated.
 * Both entry points read the same two DEVICE tables (the caller keeps host copies and validates on them):
 *   wdesc [B][8] int64: Hc, Wc, ny, nx, n0, offset of the image's origins in `origins`, two spare entries (0);
 *   origins int32: per image, at its offset, ny row origins ys[0..ny) then nx column origins xs[0..nx).
 * Along an axis of canvas length n the origins are strictly increasing, the first is 0, the last is n - S, consecutive
 * ones are at most S apart (every canvas coordinate is covered) and origins[k + 3] >= origins[k] + S (by at most
 * HRSEG_WINDOW_MAX_COVER = 3 of them); ny, nx <= HRSEG_WINDOW_MAX_ORIGINS.  The windows of image m are the tensor product
 * ys x xs, row-major, numbered n0 + a * nx + b; all numbers lie in [0, nwindows).
 *
 * hrseg_window_crops: x [nwindows,3,S,S] fp32.  Element (i, j) of window (a, b) of image m is the eval-mode value of
 * hrseg_augment_image at canvas pixel (ys[a] + i, xs[b] + j) of a resize of source m (ragged uint8, desc as for
 * hrseg_augment_image) to Hc x Wc: torch bilinear taps (align_corners=False) with scales H_m / Hc and W_m / Wc, then
 * (v - 0.5) / 0.5; a one-channel source is replicated.  With Hc = Wc = S and one window the call is hrseg_augment_image
 * (train == 0) bit for bit.  1 launch, family "window_crops", outside the NULL total; no workspace.
 *
 * hrseg_decode_windows: z: HOST array of nlevels DEVICE pointers, level L is [nwindows, C[L], S, S] fp32; profile: DEVICE
 * array of S strictly positive fp32 blend weights (the same along both axes).  For output pixel (y, x) of image m, whose
 * size H_m x W_m comes from desc (it need not be the canvas size):
 *   1. canvas taps and weights: torch bilinear taps of y at scale Hc / H_m in a source of Hc rows, of x at Wc / W_m in Wc
 *      columns -- the function and the rounding of hrseg_decode_labels; at H_m == Hc the tap is y with weight 1;
 *   2. blended logit of channel k at a canvas pixel (r, c): A = the origins a with ys[a] <= r < ys[a] + S in ascending
 *      order, Bc likewise for the columns, wy_a = profile[r - ys[a]], wx_b = profile[c - xs[b]].  In fp32, every operation
 *      rounded to nearest and none contracted:
 *        t_ab = (wy_a * wx_b) * z[n0 + a * nx + b][k][r - ys[a]][c - xs[b]]
 *        num  = the t_ab added one by one, a ascending and within a the b ascending, starting FROM the first (not from 0)
 *        sy   = the wy_a added in ascending order from the first, sx likewise
 *        g    = num / (sy * sx)                                            (IEEE division)
 *      One covering window with an all-ones profile gives (1 * 1) * z / (1 * 1) = z bit for bit;
 *   3. the 2 x 2 blend of g at the four canvas taps, along x first, with the multiplies and fused multiply-adds of
 *      hrseg_decode_labels in the same order.  A tap whose weight is 0 is not fetched: 0 takes its place;
 *   4. steps 2-5 of hrseg_decode_labels unchanged: arg-max over level 0, top-down through the chosen node's child group
 *      only, leaf pixel value, optional confidence (root_softmax as there).
 * One window per image (Hc = Wc = S) with an all-ones profile therefore returns what hrseg_decode_labels returns, bit for
 * bit.  Only the channels on the decoded path are fetched (up to 4 taps x 9 windows each), with 64-bit offsets into z.
 * Refused with a message before anything is launched: NULL pointers (confidence may be NULL), B outside 1..65535,
 * S outside 1..32768, nwindows < B, and every limit and alignment rule of hrseg_decode_labels on nlevels, C, the tree,
 * labels and confidence.  1 launch, family "decode_windows" (never "decode_labels"), outside the NULL total; no
 * workspace, no device allocation, no synchronisation. */
#define HRSEG_WINDOW_MAX_ORIGINS 64
#define HRSEG_WINDOW_MAX_COVER 3
int hrseg_window_crops(const unsigned char* src, const long* desc, const long* wdesc, const int* origins, float* x,
                       int B, int S, int nwindows, hrseg_stream_t stream);
int hrseg_decode_windows(int nlevels, const float* const* z, const int* C, const hrseg_decode_tree_t* tree,
                         const long* wdesc, const int* origins, const float* profile, const long* desc,
                         unsigned char* labels, float* confidence, int B, int S, int nwindows, hrseg_stream_t stream);

/* ------------------------------------------------------------------ device scoring pipeline (Data/score.py)
 * The third stage behind the input and output pipelines: a batch of predicted label maps (hrseg_decode_labels) against
 * ground-truth label maps at the SOURCE size, both in the pixel values of class_map.csv -> per-level confusion counts in
 * the layout hrseg_metric_vectors reads.
 * Levels are the tree's depths in breadth-first channel order, whatever model produced the map (a flat model's leaf map
 * is scored per hierarchy level the same way).  Limits as for the decode: nlevels <= 8, C[L] <= 16, sum C[L] <= 64.
 * path_lut: DEVICE table [256] of uint64 built on the host from the class tree and class map: byte L of entry v is
 * 1 + channel of the level-L node on the path from the root to the leaf whose pixel value is v, 0 when that leaf is
 * shallower than L; the whole entry is 0 when v is no leaf's value.  (An entry that names a channel above C[L], or has no
 * level-0 node, or a node at a level >= nlevels, counts as 0.)
 * pred / gt: packed uint8 buffers, pdesc / gdesc their DEVICE [B][4] int64 tables (byte offset, H, W, 1): map b is a
 * dense span of H_b * W_b bytes at its own offset in its own buffer; both tables must give the same H_b x W_b (a sample
 * where they differ, or with H*W > 2^31, is not counted at all -- the host wrapper refuses both).  For pixel i of
 * sample b, with g = path_lut[gt], p = path_lut[pred] and g_L / p_L byte L of them:
 *   - g == 0: ignored[b][0] += 1 (unlabelled ground truth), nothing else is counted;
 *   - else p == 0: ignored[b][1] += 1 (a prediction outside the class map), nothing else is counted;
 *   - level 0: cm_0[(g_0 - 1) * C_0 + (p_0 - 1)] += 1;
 *   - level L >= 1: K_L = C_L + 1, label 0 is the synthetic background; t = g_L, q = (g_{L-1} == p_{L-1}) ? p_L : 0;
 *     cm_L[t * K_L + q] += 1.
 * A prediction competes at level L only where it agreed with the ground truth at the level above: the restrictive
 * masking of the train loop (t == -1 zeroes the prediction) applied to decoded paths.  Every level's matrix therefore
 * sums to the number of valid pixels; hrseg_metric_vectors drops row 0 of the child levels.
 * DELIBERATE DEVIATION from the metrics at network size (hrseg_predict_metrics): there an unlabelled pixel lands in row 0
 * of level 0, because the arg-max of an all-zero target picks channel 0; here it is ignored and counted in `ignored`.
 * counts: DEVICE int64 [per_image ? B : 1][sum_L K_L^2] (K_0 = C_0), levels side by side, (target, predicted), +=
 * (accumulate a dataset total in place); ignored: DEVICE int64 [per_image ? B : 1][2], +=.  C is a HOST array.
 * All arithmetic is integer: the result does not depend on the block order nor on the "deterministic" knob.  One launch
 * (family "score_labels"), no workspace, no device allocation, no synchronisation.  The kernel never reads outside
 * [offset, offset + H*W) of either buffer.  A lane counts HRSEG_SCORE_LANE_STEP consecutive pixels per step. */
#define HRSEG_SCORE_MAX_LEVELS 8
#define HRSEG_SCORE_MAX_CHANNELS 16
#define HRSEG_SCORE_LANE_STEP 16
#define HRSEG_SCORE_WAVE_STEP 1024
#define HRSEG_SCORE_BLOCK_STEP 4096
int hrseg_score_labels(const unsigned char* pred, const long* pdesc, const unsigned char* gt, const long* gdesc,
                       const unsigned long long* path_lut, int nlevels, const int* C, long long* counts,
                       long long* ignored, int B, int per_image, hrseg_stream_t stream);

/* ------------------------------------------------------------------ device post-processing (Data/postprocess.py; csrc/components.hip)
 * The fourth stage: connected-component clean-up of label maps (hrseg_decode_*), on the device.  A batch is a packed uint8
 * buffer `labels` with a DEVICE table desc [B][4] int64 (byte offset, H, W, 1) exactly as hrseg_score_labels reads it:
 * image b is the dense row-major span [offset_b, offset_b + H_b * W_b); offsets are arbitrary bytes, gaps are allowed.
 * desc_host is the HOST copy of the same table: the entry points size their grids and check their limits on it, the
 * kernels read `desc`.  group: DEVICE table [256] of bytes, pixel value -> group id.
 *
 * hrseg_label_components.  A COMPONENT is a maximal 4- or 8-connected (connectivity) set of pixels OF ONE IMAGE with
 * equal group[label].  Images never connect, however they lie in the buffer.  The FIRST pixel of a component is the one
 * with the smallest row-major index y * W + x within its image.  roots and area are int32 buffers with the labels buffer's
 * own indexing (element i belongs to byte i):
 *   roots[offset + y * W + x] = row-major index of the first pixel of the pixel's component;
 *   area [offset + y * W + x] = the component's pixel count where (y, x) is that first pixel, 0 at every other pixel.
 * Elements outside every image span are not written; label bytes outside the spans are not read (rows are read through
 * aligned 16-byte loads that lie inside the span, single bytes elsewhere).
 * Method: union-find with the parent array in `roots`; a union links the larger root below the smaller, so parent[i] <= i
 * at all times, every walk descends, and the root is the smallest index whatever order the atomics land in: the result
 * is the same bytes in every run.  A block labels a tile of HRSEG_COMPONENTS_TILE_W x HRSEG_COMPONENTS_TILE_H pixels in
 * LDS (hrseg_components_tile returns the two numbers), a second launch unites across tile borders, a third flattens and
 * counts.  HRSEG_LABEL_COMPONENTS_LAUNCHES launches, counted under the family "label_components" (outside the NULL
 * total); no workspace, no device allocation, no host read, no synchronisation.
 * Refused with a message before anything is launched: NULL pointers; B outside 1..65535; connectivity not 4 or 8; roots or
 * area not 4-byte aligned; a descriptor row with a negative offset, H < 1, W < 1 or channels != 1; H * W >= 2^31.
 *
 * hrseg_filter_components.  roots / area: what hrseg_label_components wrote for the same labels, desc and group.
 * rules: DEVICE table of 256 hrseg_component_rule_t, one per group id.  A component of group g != 255 is REMOVED when
 *   area < rules[g].min_area, or
 *   rules[g].keep_largest != 0 and it is not the largest component of group g in its image (equal areas: the one whose
 *   first pixel has the smaller index is the largest).
 * Every pixel of a removed component is written to out as the fill value: rules[g].fill in 0..255, or for fill < 0 the
 * INPUT label of the west neighbour of the component's first pixel; of its north neighbour when the first pixel lies in
 * column 0; and when the first pixel is the image's origin the component stays as it is and does not count as removed.
 * (That neighbour is of another group: a west or north neighbour of the same group would belong to the component and
 * come first.  It is read from `labels`, so a neighbour that is removed itself does not cascade.)  All other pixels are
 * copied; group 255 has no rule and is always copied.  out has the layout of labels; bytes outside the spans are not
 * written; out must not overlap labels (the spans' extent from the buffers' starts).
 * stats: DEVICE int64 [B][256][3], += (the caller zeroes it): per image and group the components found, the components
 * removed, the pixels of removed components.  workspace: hrseg_filter_components_workspace_bytes(B) bytes, 8-byte
 * aligned; the call initialises it.  HRSEG_FILTER_COMPONENTS_LAUNCHES launches (clearing the workspace, the
 * per-group maximum, the filter), family "filter_components", outside the NULL total; no host read, no synchronisation.
 * Refused before anything is launched: NULL pointers; B outside 1..65535; roots, area or rules not 4-byte, stats or
 * workspace not 8-byte aligned; the descriptor rules above; out overlapping labels. */
#define HRSEG_COMPONENTS_TILE_W 64
#define HRSEG_COMPONENTS_TILE_H 32
#define HRSEG_LABEL_COMPONENTS_LAUNCHES 3
#define HRSEG_FILTER_COMPONENTS_LAUNCHES 3
typedef struct {
  int min_area;      /* components with fewer pixels are removed */
  int keep_largest;  /* != 0: all but the largest component of the group are removed */
  int fill;          /* 0..255, or < 0: the neighbour rule */
} hrseg_component_rule_t;
int hrseg_components_tile(int* w, int* h);
size_t hrseg_filter_components_workspace_bytes(int B);
int hrseg_label_components(const unsigned char* labels, const long* desc, const long* desc_host, int B,
                           const unsigned char* group, int connectivity, int* roots, int* area, hrseg_stream_t stream);
int hrseg_filter_components(const unsigned char* labels, const long* desc, const long* desc_host, int B,
                            const unsigned char* group, const hrseg_component_rule_t* rules, const int* roots,
                            const int* area, unsigned char* out, long long* stats, void* workspace,
                            hrseg_stream_t stream);

/* ------------------------------------------------------------------ device boundary scoring (Data/boundary.py; csrc/boundary.hip)
 * The fifth, optional stage: how far the predicted outline of every tree node lies from the true one.  Label maps and
 * ground-truth maps at the source's own size, both in the pixel values of class_map.csv, in the packed-buffer + [B][4]
 * descriptor form of hrseg_score_labels and hrseg_label_components -> per image and tree node the integer records from which
 * the Hausdorff distance, its percentile, the average symmetric surface distance and the surface Dice follow.  No map
 * leaves the device; no host read, no synchronisation, no device allocation.
 *
 * Nodes: all nodes of the class tree in breadth-first order (the order of the metric vectors), node = sum_{l<L} C[l] + c for
 * channel c of level L, N = sum C[L].  Limits as for hrseg_score_labels: nlevels <= 8, C[L] <= 16, N <= 64.  path_lut is the
 * table of hrseg_score_labels (byte L of entry v = 1 + channel of the level-L node of the leaf with pixel value v, 0 below
 * the leaf; an entry that breaks the rules stated there counts as 0).
 * Validity: a pixel whose ground truth is no leaf's value belongs to no node IN EITHER MAP (hrseg_score_labels counts
 * nothing there either); a predicted value outside the class map belongs to no predicted node.
 * Masks: the mask of node n at level L in a map is the set of valid pixels whose path has n in byte L.  There is NO
 * restrictive masking -- on purpose unlike hrseg_score_labels, where a prediction competes at level L only where it agreed
 * with the truth above: an outline is a property of one map.
 * Border pixels: a pixel of a mask is a border pixel when one of its FOUR neighbours is outside the mask; the outside of the
 * image counts as outside the mask.  P_n: the border pixels of node n in the prediction, G_n: in the ground truth.
 * Distance: for x in P_n, d2(x) = min over y in G_n of (dy^2 + dx^2), an exact integer; the other direction likewise.
 * H, W <= HRSEG_BOUNDARY_MAX_SIDE = 32768 keeps d2 < 2^31 (and H*W < 2^31 as elsewhere); larger maps are refused, and a
 * sample whose DEVICE descriptors break a rule, or whose two tables disagree on a size, is skipped by the kernels.
 *
 * records: DEVICE int64 [B][N][2][5], WRITTEN (not accumulated).  Direction 0: prediction -> truth (the pixels of P_n query
 * G_n), direction 1: truth -> prediction.  Fields:
 *   0 n        border pixels of the querying set;
 *   1 sum_q16  sum over those pixels of floor(sqrt(d2 << 32)): the distance in 16.16 fixed point, floored (Python:
 *              math.isqrt(d2 << 32)).  Integer, so the sum is exact whatever order the atomics land in; on the device a
 *              floating-point root is only the first guess, corrected with integer multiplies;
 *   2 max_d2   the largest d2;
 *   3 within   pixels with d2 <= tau2; the caller computes tau2 = floor(tolerance^2);
 *   4 pk_d2    the k-th smallest d2, k = ceil(percentile * n / 100) = (percentile * n + 99) / 100 in integers: the
 *              NEAREST-RANK percentile, no interpolation, per direction.
 * When n is 0 in EITHER direction (the node is absent from one map or from both) every field but the two n is 0.
 * The usual figures follow (Data/boundary.py derives them, NaN where either n is 0):
 *   hausdorff = sqrt(max(max_d2[0], max_d2[1])),  hd_percentile = sqrt(max(pk_d2[0], pk_d2[1])),
 *   assd = (sum_q16[0] + sum_q16[1]) / 65536 / (n[0] + n[1]),  surface_dice = (within[0] + within[1]) / (n[0] + n[1]).
 * DELIBERATE CONVENTION: hd_percentile is the larger of the two directions' nearest-rank percentiles.  Some libraries take
 * numpy's linearly interpolated percentile of the two directions' distances concatenated instead; the two differ by up to
 * the gap between neighbouring order statistics, and where the two sets have very different sizes.
 *
 * desc_host: HOST table [2][B][4]: the host copy of pdesc's B rows followed by that of gdesc's; the entry point sizes its
 * grids and checks its limits on it, the kernels read pdesc / gdesc.  C is a HOST array.
 * workspace: hrseg_boundary_workspace_bytes(desc_host, B, nlevels, C) bytes (it reads the first B rows; 0 with a message
 * when an argument is refused), 8-byte aligned, DEVICE; the call's own first launch initialises what it needs of it, so a
 * dirty workspace may be reused.  In bytes: 16 B + 4 * (B * 2 N * HRSEG_BOUNDARY_SEGMENT_WORDS + bitmaps + maps), bitmaps =
 * sum_b 2 N H_b ceil(W_b / 32) rounded up to an even number, maps = sum_b 2 nlevels H_b W_b: one border bitmap per
 * (node, map) with rows padded to 32-bit words (tail bits stay 0), one int32 d2 map per (level, direction), and 256 radix
 * bins per (image, node, direction).
 * Method (csrc/boundary.hip): mark the border bitmaps of all nodes in one pass over both maps; every border pixel searches
 * the other map's bitmap of its own node -- the 7 rows around it first, which decides every d2 <= 16, else row by row outwards
 * with a whole wave on the query until the vertical offset alone exceeds the best distance; the k-th smallest per (image, node, direction) by four 8-bit radix passes over the d2 maps.  Reads never
 * leave [offset, offset + H*W) of either buffer.  HRSEG_SCORE_BOUNDARIES_LAUNCHES launches, family "score_boundaries",
 * outside the NULL total.  All arithmetic is integer: the same bytes in every run, whatever the "deterministic" knob says.
 * Refused with a message before anything is launched: NULL pointers; B outside 1..65535; records, workspace or path_lut
 * not 8-byte aligned; percentile outside 1..100; tau2 < 0; nlevels / C outside the limits; a descriptor row (of either
 * table) with a negative offset, H < 1, W < 1 or channels != 1, H * W >= 2^31 or a side above 32768; the two tables
 * disagreeing on a size. */
#define HRSEG_SCORE_BOUNDARIES_LAUNCHES 11
#define HRSEG_BOUNDARY_MAX_SIDE 32768
#define HRSEG_BOUNDARY_SEGMENT_WORDS 260
size_t hrseg_boundary_workspace_bytes(const long* desc_host, int B, int nlevels, const int* C);
int hrseg_score_boundaries(const unsigned char* pred, const long* pdesc, const unsigned char* gt, const long* gdesc,
                           const long* desc_host, const unsigned long long* path_lut, int nlevels, const int* C, long tau2,
                           int percentile, long long* records, void* workspace, int B, hrseg_stream_t stream);

/* ------------------------------------------------------------------ device instance scoring (Data/instances.py; csrc/instances.hip)
 * The sixth, optional stage: the question per OBJECT -- how many teeth, restorations or lesions were found, missed or
 * invented, and how well each found one overlaps its true one.  The connected components (hrseg_label_components) of the
 * prediction and of the ground truth are matched one to one on the device -> per image and group of the cut the integer
 * records from which detection precision / recall / F1, segmentation quality and panoptic quality (PQ = SQ x RQ) follow,
 * and per-instance match maps.  No map leaves the device; no host read, no synchronisation, no device allocation.
 *
 * Inputs as for hrseg_score_labels / hrseg_score_boundaries: packed uint8 buffers pred and gt with their DEVICE [B][4] int64
 * tables pdesc / gdesc (byte offset, H, W, 1) -- arbitrary offsets and gaps, the two buffers may be laid out differently, the
 * two tables must agree on every H_b x W_b -- and desc_host, the HOST table [2][B][4]: the host copy of pdesc's B rows
 * followed by that of gdesc's.  The entry points size their grids and check their limits on desc_host, the kernels read
 * pdesc / gdesc; a sample whose DEVICE descriptors break a rule, disagree on the size or leave the extent of the host
 * table is skipped by the kernels.
 * group: the DEVICE [256] byte table of hrseg_label_components (pixel value -> group id of the cut, 255 = no leaf's value).
 * things: DEVICE [256] bytes, non-zero for the group ids that are scored as instances; group 255 is never a thing.
 *
 * Validity.  A pixel whose ground-truth value has group 255 is VOID: it belongs to no component IN EITHER MAP (the convention
 * of hrseg_score_boundaries).  A predicted value of group 255 belongs to no predicted component.
 * hrseg_mask_void_labels realises this by a masked copy of the prediction: out[i] = pred[i] where the ground truth is valid,
 * else void_value, a byte the caller picks with group[void_value] == 255; void_value = -1: no such byte exists, nothing can
 * be void and out is a plain copy.  group is device memory, so THE CALLER checks group[void_value] == 255 (ops.mask_void_labels
 * does, on the host table it builds the device table from); the entry point checks the range -1..255.  out has the layout
 * of pred and must not overlap it; bytes outside the spans are neither read nor written.  One launch.
 * Components are those of hrseg_label_components on the masked prediction pm and on gt, with one group table and one
 * connectivity.  DELIBERATE CONVENTION: a predicted region cut in two by a void area is TWO components, one lying wholly in
 * void does not exist.
 *
 * Match.  A predicted component P and a true component G of the same thing group in the same image, inter = |P n G|,
 * match when 3 * inter > |P| + |G|: IoU = inter / (|P| + |G| - inter) > 1/2 in integers; IoU exactly 1/2 does not match.
 * At most one partner exists on either side: |P| >= inter gives 2 * inter > |G|, so a partner holds more than half of G's
 * pixels, and two disjoint components cannot both; likewise for P.
 *
 * hrseg_score_instances.  pm / proots / parea and gt / groots / garea: the masked prediction and the ground truth with the
 * roots and areas hrseg_label_components wrote for them (same desc tables, group and connectivity).
 * records: DEVICE int64 [per_image ? B : 1][256][HRSEG_INSTANCE_FIELDS], indexed by group id, ACCUMULATED (+=; the caller
 * zeroes it, a dataset total accumulates in place as for hrseg_score_labels).  Rows of groups that are no things are not
 * touched.  Fields:
 *   0 n_gt, 1 n_pred    the thing components of the ground truth / of the masked prediction;
 *   2 tp                the matched pairs;  fp = n_pred - tp, fn = n_gt - tp;
 *   3 sum_iou_q30       sum over the matched pairs of floor((inter << 30) / union), union = |P| + |G| - inter, unsigned
 *                       64-bit: an integer, so the sum is exact in any order;
 *   4 sum_inter, 5 sum_union   over the matched pairs;
 *   6..9 tp_at[k]       the matched pairs with inter * 1000 >= thresholds[k] * union.
 * thresholds: HOST int[4], per mille; 0 = unused (the field stays as it was), else 501..1000.
 * gmatch, ginter: int32, indexed like the gt buffer; pmatch: int32, indexed like the prediction buffer.  Inside the image
 * spans every element is written: gmatch / pmatch hold at the FIRST pixel of a thing component the row-major index (within
 * the image) of the partner's first pixel, or -1 when unmatched, and -2 everywhere else; ginter holds inter at the first
 * pixel of a matched true component and 0 elsewhere.  Elements outside every span are not written, bytes outside the
 * spans are not read.
 * workspace: hrseg_instances_workspace_bytes(desc_host, B) bytes (it takes the same [2][B][4] table and reads the
 * ground-truth rows; 0 with a message when refused), 8-byte aligned, DEVICE: with E = the extent of the ground-truth buffer
 * (max_b offset_b + H_b W_b), 8 E bytes of vote slots + 4 E of overlaps, rounded up to 8 -- below 16 bytes per byte of the
 * extent, computed on the host; nothing is sized by a component count.  The call's first launch initialises what it needs,
 * so a dirty workspace may be reused.
 * Method (csrc/instances.hip).  No pair table: the distinct (P, G) pairs are bounded by the pixel count only.  Every true
 * thing component has one 64-bit slot (candidate root, count) at its first pixel's index; every pixel of G votes for the
 * predicted component of G's group it lies in, or for "none", as runs of equal (g_root, p_root) merged into weighted votes;
 * a Boyer-Moore majority vote is merged into the slot by a compare-and-swap loop (an empty slot takes the vote, an equal
 * candidate adds, another subtracts, what passes zero takes over).  The loop serialises the votes in SOME order, a weighted
 * vote equals its unit votes in sequence, and a strict majority is the final candidate in every order.  A second pass
 * counts inter with the candidate, a third applies the exact test: where a partner exists it is the candidate, where none
 * exists every candidate fails -- the same bytes in every run although the vote's intermediate state is not, and whatever
 * the "deterministic" knob says.  HRSEG_SCORE_INSTANCES_CALL_LAUNCHES launches; with the masked copy's one the stage
 * counts HRSEG_SCORE_INSTANCES_LAUNCHES under the family "score_instances", outside the NULL total (the two labellings
 * count under "label_components").
 * Refused with a message before anything is launched, under the entry point's own name: NULL pointers; B outside 1..65535;
 * roots, areas, pmatch, gmatch or ginter not 4-byte, records or workspace not 8-byte aligned; a descriptor row of either
 * table with a negative offset, H < 1, W < 1 or channels != 1; H * W >= 2^31; the two tables disagreeing on a size; a
 * threshold outside {0, 501..1000}; void_value outside -1..255; out overlapping pred (the spans' extent from the buffers'
 * starts). */
#define HRSEG_INSTANCE_FIELDS 10
#define HRSEG_MASK_VOID_LABELS_LAUNCHES 1
#define HRSEG_SCORE_INSTANCES_CALL_LAUNCHES 4
#define HRSEG_SCORE_INSTANCES_LAUNCHES (HRSEG_MASK_VOID_LABELS_LAUNCHES + HRSEG_SCORE_INSTANCES_CALL_LAUNCHES)
size_t hrseg_instances_workspace_bytes(const long* desc_host, int B);
int hrseg_mask_void_labels(const unsigned char* pred, const long* pdesc, const unsigned char* gt, const long* gdesc,
                           const long* desc_host, const unsigned char* group, int void_value, unsigned char* out, int B,
                           hrseg_stream_t stream);
int hrseg_score_instances(const unsigned char* pm, const long* pdesc, const int* proots, const int* parea,
                          const unsigned char* gt, const long* gdesc, const int* groots, const int* garea,
                          const long* desc_host, const unsigned char* group, const unsigned char* things,
                          const int* thresholds, long long* records, int* pmatch, int* gmatch, int* ginter, void* workspace,
                          int B, int per_image, hrseg_stream_t stream);

/* ------------------------------------------------------------------ device calibration scoring (Data/calibration.py; csrc/calibration.hip)
 * The fourth scorer: does the model's composed probability mean anything?  Per-level logits at network size against
 * ground-truth label maps at the SOURCE size -> per tree node, and per level for the decoded path's top label, a reliability
 * histogram of exact integers from which ECE, MCE and the Brier score follow on the host.  No full-size probability plane
 * exists at any point.
 * z, C, tree and S as for hrseg_decode_labels; gt, gdesc and path_lut as for hrseg_score_labels (an entry of path_lut that
 * names a channel above C[L], has no level-0 node or a node at a level >= nlevels counts as 0).  inv_temp: HOST array of
 * nlevels floats, 1 / temperature per level.  Rows: R = sum_L C[L] + nlevels; the node rows first, in breadth-first channel
 * order (level 0's channels, then level 1's, ...), then the nlevels "top-label" rows.  For pixel (y, x) of sample b (H_b x W_b
 * from gdesc):
 *   1. g = path_lut[gt byte]; g == 0: ignored[per_image ? b : 0] += 1 and nothing else happens;
 *   2. EVERY logit of EVERY level is resampled S x S -> H_b x W_b with the same multiplies and adds, in the same order, as
 *      hrseg_decode_labels step 1 (the same taps and weights, every product and sum rounded on its own), then multiplied
 *      once (one rounding) by inv_temp[L]: v_L[c].  inv_temp[L] == 1.0f is the identity bit for bit;
 *   3. node probabilities are the model's own composition: P_0[c] = sigmoid(v_0[c]) (with root_softmax: the soft-max over
 *      level 0); P_L[c] = P_{L-1}[parent(c)] * softmax_group(v_L)[c] for L >= 1, parent and groups from first_child /
 *      n_children.  A channel of level L+1 that is in no child group (or in two) is refused before launch;
 *   4. the decoded path c_0, c_1, ... is exactly that of hrseg_decode_labels (arg-max of the logits, strict >, lowest index
 *      wins); T_L = P_L[c_L] for every level the path reaches;
 *   5. events (p, y): node row (L, c): p = P_L[c], y = (byte L of g) - 1 == c -- one event per valid pixel, always (a leaf
 *      shallower than L has byte 0 there: y = 0).  Top row L: only where the path reaches level L AND byte L of g is
 *      non-zero: p = T_L, y = (c_L == byte L of g - 1).  A pixel where exactly one of the two -- decoded path, ground
 *      truth -- has a node at level L produces NO top-label event (hrseg_score_labels counts those pixels, in row or
 *      column 0 of its level matrix);
 *   6. an event goes to hist[img][row][bin][4] = (n, pos, sum_q, sum_e2), int64, +=, n_bins + 1 bins per row:
 *      q = (unsigned)rintf(clamp(p, 0, 1) * 16777216.f); bin = min(n_bins - 1, (q * n_bins) >> 24);
 *      e = y ? 16777216 - q : q; e12 = (e + 2048) >> 12; the cell gets n += 1, pos += y, sum_q += q, sum_e2 += e12 * e12.
 *      A NaN p goes to the extra bin n_bins with n and pos only (tested before the clamp, which would swallow it), so the
 *      sum over all n_bins + 1 bins of n is the row's event count exactly and a non-finite logit stays visible.
 * Capacity: sum_q <= 2^24 N and sum_e2 <= 2^24 N for N events, so a dataset total of 2^39 events per cell fits an int64.
 * That is why the squared error is taken on a 2^-12 grid: the square of a 2^-24 error is up to 2^48, which overflows int64
 * after 2^15 events -- inside one large image.
 * hist: DEVICE int64 [per_image ? B : 1][R][n_bins + 1][4]; ignored: DEVICE int64 [per_image ? B : 1]; both += (a dataset total
 * accumulates in place).  Everything accumulated is an integer: the result depends neither on the block order nor on the
 * "deterministic" knob.  One launch (family "score_calibration", outside the NULL total), no workspace, no device
 * allocation, no synchronisation.  The kernel never reads outside [offset, offset + H*W) of gt.  A sample with H*W > 2^31
 * is not counted at all (the host wrapper refuses it).
 * Refused with a message before anything is launched: null pointers; B outside 1..65535; S outside 1..32768; n_bins outside
 * 1..HRSEG_CALIBRATION_MAX_BINS; hist, ignored or path_lut not 8-byte aligned; every limit of hrseg_decode_labels on nlevels,
 * C and the tree (nlevels <= 8, C[L] <= 16, sum <= 64); an inv_temp[L] that is not finite and > 0; an uncovered channel. */
#define HRSEG_CALIBRATION_MAX_BINS 32
int hrseg_score_calibration(int nlevels, const float* const* z, const int* C, const hrseg_decode_tree_t* tree,
                            const float* inv_temp /* HOST [nlevels] */, const unsigned char* gt, const long* gdesc,
                            const unsigned long long* path_lut, int n_bins, long long* hist, long long* ignored,
                            int B, int S, int per_image, hrseg_stream_t stream);

/* ------------------------------------------------------------------ consensus (Data/consensus.py; csrc/consensus.hip)
 * Several label maps of the same images -> one, voted down the class tree, plus the integer counters every inter-map
 * agreement figure follows from.  The maps may say less than a leaf per pixel: internal nodes' bytes (hrseg_decode_hedged,
 * partial labels) and bytes that say nothing at all.
 *
 * Inputs.  M member batches, 1 <= M <= HRSEG_CONSENSUS_MAX_MEMBERS.  Each member is a packed uint8 buffer of B ragged maps
 * in the descriptor format of hrseg_score_labels ([B][4] int64: byte offset, H, W, 1; offsets are arbitrary bytes, gaps are
 * allowed).  members: HOST array of M DEVICE pointers (like z of the decodes).  desc: ONE DEVICE table [M][B][4], member
 * m's rows at desc + 4 B m; desc_host its HOST copy (the [2][B][4] pair convention of the scorers, extended to M).  Every
 * member must give the same H_b x W_b for sample b.  path_lut: DEVICE [256] uint64 in exactly the format of
 * hrseg_score_labels, INCLUDING entries that end at an internal node (zero bytes below it); the entry rule stated there
 * applies unchanged.  An entry of 0 (reject byte, ignore byte, foreign byte) means: this member ABSTAINS at this pixel.
 * The tree, the output bytes and the quorum travel in hrseg_consensus_t (a kernel argument: no device table).
 *
 * Per pixel, with e_m the path entry of member m's byte:
 *   votes[L][c] = the number of members whose byte L of e_m equals c + 1.  A member that names a child has named its
 *     parent, so votes never grow down a path (no restriction to "members who agreed above" is needed).
 *   quorum q is an absolute count with 2 q > M and q <= M.  An abstention counts against a node -- deliberately: the
 *     denominator is M.  Each member names at most one node per level and 2 q > M, so at most one node per level reaches q:
 *     the nodes that reach q form one chain from a root.
 *   The CONSENSUS NODE is the deepest node of that chain.  labels[offset + i] = out_val[L][c] of that node (a leaf's pixel
 *     value, or an internal node's byte); none_val if no level-0 node reaches q.
 *   support (optional, may be NULL; uint8, packed as labels): the votes of the consensus node, 0 where labels is none_val.
 * Both outputs are packed as MEMBER 0 is: pixel i of sample b lies at the byte offset of row b of member 0's table.
 * Worked example, M = 3, q = 2: (tooth, enamel, enamel) -> tooth has 3 votes, enamel 2: enamel.  (enamel, dentin, tooth)
 * -> tooth 3, enamel 1, dentin 1: the byte of "tooth".  (upper-tooth, lower-tooth, reject) -> no root reaches 2: none_val.
 *
 * Counters: DEVICE int64 [per_image ? B : 1][cells], += (a dataset total accumulates in place).  N = sum C nodes in
 * breadth-first channel order (node = sum_{l<L} C[l] + c), P = M (M - 1) / 2 pairs i < j in lexicographic order.  The cells
 * of a row, in this order:
 *   ended    N + 1   pixels whose consensus ended ON each node, then "none"
 *   votes    N x M   votes[n][k-1] = pixels where exactly k members have node n on their path, k = 1..M (k = 0 follows on
 *                    the host)
 *   area     M x N   pixels where member m has node n on its path
 *   both     P x N   pixels where both members of the pair have node n on their path
 *   abstain  M       pixels where member m's entry is 0
 * cells = N + 1 + 2 N M + P N + M <= 2889.  Everything is integer arithmetic: the same bytes in every run, independent of
 * the block order and of the "deterministic" knob.
 *
 * One launch, family "consensus_labels", outside the NULL total.  No workspace, no device allocation, no synchronisation,
 * no host read.  The kernel never reads outside [offset, offset + H*W) of any member and never writes outside the output
 * spans.  A block takes HRSEG_CONSENSUS_BLOCK_STEP pixels per step, a lane HRSEG_CONSENSUS_LANE_STEP consecutive ones.
 * Refused, each before any launch, with -1 and a message that starts with the entry point's name: null required pointers
 * (members and each of its M entries, desc, desc_host, path_lut, cons, labels, counts); B outside 1..65535; M outside
 * 1..8; 2 q <= M or q > M; nlevels outside 1..8, a C[L] outside 1..16, sum C > 64; an out_val of an existing node or
 * none_val outside 0..255, or any two of them equal; a host descriptor row with a negative offset, H < 1, W < 1,
 * channels != 1 or H * W >= 2^31; members that disagree on a size (the message names the member, the image and both
 * sizes); counts or path_lut not 8-byte aligned; labels not 4-byte aligned (the rule of the decodes' labels).  Entries of
 * out_val beyond the tree's channels are not read. */
#define HRSEG_CONSENSUS_MAX_MEMBERS 8
#define HRSEG_CONSENSUS_LANE_STEP 16
#define HRSEG_CONSENSUS_BLOCK_STEP 4096
typedef struct {
  int nlevels;
  int C[HRSEG_SCORE_MAX_LEVELS];                                    /* channels per level */
  int out_val[HRSEG_SCORE_MAX_LEVELS][HRSEG_SCORE_MAX_CHANNELS];    /* the byte written where the consensus ends ON node (L, c) */
  int none_val;                                                     /* the byte written where no level-0 node reaches the quorum */
  int quorum;                                                       /* absolute count: 2 * quorum > M, quorum <= M */
} hrseg_consensus_t;
int hrseg_consensus_labels(int M, const unsigned char* const* members, const long* desc, const long* desc_host,
                           const unsigned long long* path_lut, const hrseg_consensus_t* cons, unsigned char* labels,
                           unsigned char* support, long long* counts, int B, int per_image, hrseg_stream_t stream);

/* ------------------------------------------------------------------ level synthesis for flat models (evaluation side; csrc/targets.hip)
 * predictEval.py:85-129 get_parent_masks (parent = union of its descendant leaves, "any > 0") and :134-185
 * combine_levels (per-level tensors stitched from leaf and parent channels).  out[b][o] is the COPY of the single
 * input channel selected by masks[o] (is_union[o] == 0) or 1.0 where any selected input channel is > 0, else 0.0.
 * Input channel i < C0 is plane i of x0, else plane i - C0 of x1 (x1 may be NULL with C1 == 0).  NCHW planes;
 * masks / is_union are HOST arrays of Cout entries; C0 + C1 <= 64, Cout <= 64. */
int hrseg_combine_levels(const float* x0, int C0, const float* x1, int C1, const unsigned long long* masks,
                         const int* is_union, float* out, int B, int Cout, long hw, hrseg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HRSEG_H */
