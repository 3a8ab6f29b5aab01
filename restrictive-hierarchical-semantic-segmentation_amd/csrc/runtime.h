// The library's two registries (runtime.hip holds the storage and the C ABI over them): the launch-counter families behind
// hrseg_launch_count and the tuning knobs behind hrseg_tune.  A family or a knob is ONE row here; the enum, the name table,
// the storage and the lookup are generated from the rows.  Included by common.h.
#pragma once

// ---- launch counters per kernel family (hrseg_launch_count): the parity tests assert that a case really ran the family
// it claims to pin (e.g. the wave-specialised kernels on a 64x64 golden with lowered routing thresholds).
// X(identifier, name, counts towards the all-families total).  The total (family == NULL) counts convolution LAUNCHES:
// "ws_canvas" counts PROBLEMS laid out as a canvas inside ws / ws_group launches, "wgrad_sp_t5" the "wgrad_sp" launches that
// used 80 x 80 tiles, the augment families (augment.hip) are the input pipeline's, "decode_labels" (decode.hip) the output
// pipeline's, "score_labels" (score.hip) the scoring pipeline's, "decode_views" / "flip_views" (decode_views.hip) the
// test-time-augmentation decode's and its input mirroring's, "window_crops" / "decode_windows" (windows.hip) sliding-window
// inference's crops and blend-decode, "ohem" (loss_ohem.hip, loss.hip) every launch that exists only with online hard example
// mining on: scores, the selection's seven, the masked loss instances, "label_components" / "filter_components"
// (components.hip) the post-processing's labelling and filter launches, "score_boundaries" (boundary.hip) the boundary
// scoring's, "score_instances" (instances.hip) the instance scoring's masked copy and its four scoring launches,
// "score_calibration" (calibration.hip) the calibration scoring's one launch, "decode_hedged" (decode_hedged.hip) the hedged
// decode's one launch per call, "mix" (mix.hip) the kernel launches of the mixing augmentation: one per entry point,
// "border_weights" (border_weight.hip) the two launches of a border weight map: label extraction and search,
// "consensus_labels" (consensus.hip) the one launch of a vote over several label maps, "tree_kl" (distill.hip) the one launch
// of a tree distillation call, forward or backward.
#define HRSEG_FAMILIES(X)                   \
  X(WS, "ws", 1)                            \
  X(WS_GROUP, "ws_group", 1)                \
  X(PATCH_SP, "patch_sp", 1)                \
  X(SP_IM2COL, "sp_im2col", 1)              \
  X(SP_PGROUP, "sp_pgroup", 1)              \
  X(SP_GROUP, "sp_group", 1)                \
  X(F32, "f32", 1)                          \
  X(F32_GROUP, "f32_group", 1)              \
  X(WGRAD_SP, "wgrad_sp", 1)                \
  X(WGRAD_F32, "wgrad_f32", 1)              \
  X(WGRAD_F32_GROUP, "wgrad_f32_group", 1)  \
  X(WGRAD9, "wgrad9", 1)                    \
  X(SMALL_CIN, "small_cin", 1)              \
  X(SP_WIDE, "sp_wide", 1)                  \
  X(WS_CANVAS, "ws_canvas", 0)              \
  X(WGRAD_SP_GROUP, "wgrad_sp_group", 1)    \
  X(WGRAD_SP_T5, "wgrad_sp_t5", 0)          \
  X(WGRAD_SP_WIDE, "wgrad_sp_wide", 1)      \
  X(AUG_IMAGE, "augment_image", 0)          \
  X(AUG_TARGETS, "augment_targets", 0)      \
  X(DECODE_LABELS, "decode_labels", 0)      \
  X(SCORE_LABELS, "score_labels", 0)        \
  X(DECODE_VIEWS, "decode_views", 0)        \
  X(FLIP_VIEWS, "flip_views", 0)          \
  X(WINDOW_CROPS, "window_crops", 0)      \
  X(DECODE_WINDOWS, "decode_windows", 0)  \
  X(OHEM, "ohem", 0)                      \
  X(LABEL_COMPONENTS, "label_components", 0)  \
  X(FILTER_COMPONENTS, "filter_components", 0)  \
  X(SCORE_BOUNDARIES, "score_boundaries", 0)  \
  X(SCORE_INSTANCES, "score_instances", 0)  \
  X(SCORE_CALIBRATION, "score_calibration", 0)  \
  X(DECODE_HEDGED, "decode_hedged", 0)  \
  X(MIX, "mix", 0)  \
  X(BORDER_WEIGHTS, "border_weights", 0)  \
  X(CONSENSUS_LABELS, "consensus_labels", 0)  \
  X(TREE_KL, "tree_kl", 0)
#define HRSEG_X(id, name, conv) CNT_##id,
enum { HRSEG_FAMILIES(HRSEG_X) CNT_N };
#undef HRSEG_X
extern long hrseg_g_cnt[CNT_N];
static inline void hrseg_count(int id, long n = 1) { hrseg_g_cnt[id] += n; }

// ---- tuning knobs (hrseg_tune): the overrides the sweep tools under tools/ and the parity tests use.
// X(key, default, restore, meaning): the knob `key` lives in `int hrseg_g_<key>`; restore = 1: a value <= 0 puts the default
// back (the routing thresholds, where 0 is no usable setting); everywhere else 0 is stored as given and, for the plan
// overrides, means "automatic".
#define HRSEG_KNOBS(X)                                                                                                               \
  X(igemm_wtm, 0, 0, "fp32 implicit GEMM: pixel tiles per wave (1, 2, 4; +10 = 96-channel tiles)")                                   \
  X(igemm_kc, 0, 0, "fp32 implicit GEMM: 16-channel chunks per K stage")                                                             \
  X(igemm_db, 0, 0, "fp32 implicit GEMM: LDS buffers")                                                                               \
  X(igemm_ksplit, 0, 0, "fp32 implicit GEMM: split-K factor")                                                                        \
  X(group_wtm, 0, 0, "grouped launches: pixel tile, 1 = 64, 2 = 128 pixels")                                                         \
  X(wgrad_pix, 0, 0, "weight gradient: pixels per stage")                                                                            \
  X(wgrad_db, 0, 0, "weight gradient: LDS buffers")                                                                                  \
  X(wgrad_blocks, 0, 0, "weight gradient: target grid")                                                                              \
  X(wgrad_group_mult, 0, 0, "grouped weight gradient: blocks per problem = clamp(mult * tiles, min, max)")                           \
  X(wgrad_group_min, 0, 0, "  ... its lower clamp (automatic: 768)")                                                                 \
  X(wgrad_group_max, 0, 0, "  ... its upper clamp (automatic: 2048)")                                                                \
  X(sp_wtm, 0, 0, "split-precision plan: pixel tiles per wave")                                                                      \
  X(sp_wtn, 0, 0, "split-precision plan: channel tile in 16-channel units; set, it keeps every problem off the wave-specialised body") \
  X(sp_ksplit, 0, 0, "split-precision plan: split-K factor")                                                                         \
  X(sp_patch, 1, 0, "0 = never use the halo-patch body")                                                                             \
  X(sp_persist, 2, 0, "persistent patch blocks per CU (0 = one tile per block)")                                                     \
  X(sp_ws, 1, 0, "0 = never use the wave-specialised body")                                                                          \
  X(sp_ws_waste, 200, 0, "wave-specialised body: tile padding accepted, percent of the image")                                       \
  X(small_cin3, 1, 0, "0 = the 3-channel 3x3 first layer stays on the generic Cin <= 8 kernels (conv_small.hip)")                    \
  X(sp_ws_bf16, 1, 0, "0 = the bf16 arithmetic (one piece, one product) stays off the wave-specialised kernels")                     \
  X(sp_ws_n48, 1, 0, "0 = 48-channel tilings stay on the block-synchronous kernels")                                                 \
  X(sp_img, 1, 0, "0 = the block-synchronous patch body splits its weights on the fly")                                              \
  X(wgrad9, 1, 0, "0 = never use the nine-tap weight-gradient kernel")                                                               \
  X(ws_epi_early, 1, 0, "0 = the wave-specialised body reads accumulate / residual values at the tile's end")                        \
  X(exp_nosplit_x, 0, 0, "MEASUREMENT ONLY -- the ceiling of 'activations pre-split in HBM' (results wrong)")                        \
  X(x_split, 1, 0, "0 = hrseg_conv_x_split_ok always answers no (activations stay fp32 everywhere)")                                 \
  X(ws_epi_cost, 0, 0, "grouped wave-specialised launch: a tile's epilogue in slab times (0 = default, negative = none; conv.hip)")   \
  X(ws_epi_acc_cost, 0, 0, "  ... of an accumulating / residual epilogue")                                                           \
  X(wgrad9_blocks, 0, 0, "nine-tap weight gradient: target blocks per problem (0 = the table in conv.hip)")                          \
  X(wgrad9_blocks1, 0, 0, "  ... for a call of one problem")                                                                         \
  X(wgrad9_blocks2, 0, 0, "  ... of two")                                                                                            \
  X(wgrad9_blocks3, 0, 0, "  ... of three")                                                                                          \
  X(wgrad9_blocks4, 0, 0, "  ... of four")                                                                                           \
  X(sp_wide, 1, 0, "0 = never use the wide-tile im2col body, 2 = also on short reductions (tests)")                                  \
  X(sp_ws_canvas, 5, 0, "canvas tiling of small images: least cut of the padded area, percent (0 = per-image tiles everywhere)")     \
  X(wgrad_group_sp, 1, 0, "0 = grouped tap-per-block weight gradients stay on the fp32 kernel")                                      \
  X(wgrad_sp_t5, 1, 0, "0 = no 80 x 80 tiles in the tap-per-block weight gradient")                                                  \
  X(wgrad_sp_wide, 1, 0, "0 = never the wide-tile weight-gradient body")                                                             \
  X(sp_wide_min_blocks, 256, 0, "wide-tile im2col body: least number of 128-pixel blocks")                                           \
  X(sp_patch_min_tiles, 192, 1, "routing threshold: least tile count of the halo-patch body")                                        \
  X(auto_min_pixels, 8192, 1, "routing threshold: HRSEG_CONV_AUTO runs fp16x2 from this many output pixels on")                      \
  X(sp_ws_min_tiles, 96, 1, "routing threshold: least tile count of the wave-specialised body")                                      \
  X(deterministic, 0, 0, "1 = every float reduction with a run-dependent order takes its single-adder form (common.h)")             \
  X(bwd_multi_slab, 0, 0, "multi-target bilinear transpose: channels of a slab of the streaming body (0 = automatic, < 0 = the gather body)") \
  X(bwd_multi_bands, 0, 0, "  ... its bands of target rows per image (0 = automatic; clamped to the coarsest target's rows)")        \
  X(fuse_bwd_multi, 1, 0, "0 = the fuse layers' backward transposes each low-resolution term in a launch of its own (engine.py)")
#define HRSEG_X(key, def, restore, meaning) extern int hrseg_g_##key;
HRSEG_KNOBS(HRSEG_X)
#undef HRSEG_X
