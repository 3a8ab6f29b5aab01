// What the decode kernels share (decode.hip: one view, decode_views.hip: the mean logit of several views, windows.hip: the
// blend of overlapping windows): the tile shape, the bilinear taps of one output coordinate, the arithmetic of a channel step and,
// on the host, the validation and packing of the tree and the prelude and launch of the three entry points.
#pragma once
#include "labelmap_common.h"      // u8 / u32 / u64; calibration.hip and decode_hedged.hip also take its label-map helpers

#define DEC_TPB 256
#define DEC_PX 4                                  // pixels per lane: one dword of labels
#define DEC_ROWS (DEC_TPB / HRSEG_WAVE)           // rows per tile: one per wave
#define DEC_TILE_W (HRSEG_WAVE * DEC_PX)
#define DEC_NODES (HRSEG_DECODE_MAX_LEVELS * HRSEG_DECODE_MAX_CHANNELS)

// torch upsample_bilinear2d (align_corners=False) source taps and weights of one output coordinate.  The source
// coordinate is ONE fused multiply-add, written out (it is what the compiler made of scale * (dst + 0.5) - 0.5 in
// decode_labels_kernel all along) so that both kernels round it alike wherever the call is inlined.
struct DecLin { int i0, i1; float l0, l1; };
__device__ __forceinline__ DecLin dec_lin(int dst, float scale, int in) {
#pragma clang fp contract(off)
  float real = __builtin_fmaf(scale, (float)dst + 0.5f, -0.5f);
  if (real < 0.f) real = 0.f;
  DecLin r;
  r.i0 = min((int)real, in - 1);
  const float lam = fminf(fmaxf(real - (float)r.i0, 0.f), 1.f);
  r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
  r.l1 = lam;
  r.l0 = 1.f - lam;
  return r;
}

// The float arithmetic of a channel step, shared by decode_views.hip and windows.hip (contraction off: every unit rounds alike).
// the 2 x 2 blend of one logit: along x first (taps p.0 / p.1 with weights lx0 / lx1), then along y
__device__ __forceinline__ float dec_blend2(float p0, float p1, float l0, float l1) {      // one axis of it
#pragma clang fp contract(off)
  return __builtin_fmaf(p0, l0, p1 * l1);
}
__device__ __forceinline__ float dec_blend(float p00, float p01, float p10, float p11, float lx0, float lx1, float ly0, float ly1) {
  return dec_blend2(dec_blend2(p00, p01, lx0, lx1), dec_blend2(p10, p11, lx0, lx1), ly0, ly1);
}

// one channel (index k, logit v) of a group's online arg-max and soft-max denominator
__device__ __forceinline__ void dec_step(float v, int k, bool want_sum, float& best, float& sum, int& arg) {
#pragma clang fp contract(off)
  if (v > best) {                                           // strict: the lowest index wins ties (torch.argmax)
    if (want_sum) sum = __builtin_fmaf(sum, expf(best - v), 1.f);
    best = v;
    arg = k;
  } else if (want_sum) {
    sum += v == best ? 1.f : expf(v - best);                // equal also covers -inf against -inf (no NaN)
  }
}

// a group's confidence factor: its soft-max at the winner, or the sigmoid of the winner (level 0 of a tree model)
__device__ __forceinline__ float dec_factor(bool want_sum, float best, float sum) {
#pragma clang fp contract(off)
  return want_sum ? 1.f / sum : 1.f / (1.f + expf(-best));
}

// Checks nlevels, C and the tree against the limits of include/hrseg.h and packs one dword per node into node[DEC_NODES]
// (bits 0-7 first child channel at the next level, 8-15 child count (0 = leaf), 16-23 leaf pixel value) and the channel
// counts into Cout[HRSEG_DECODE_MAX_LEVELS].  `who` is the entry point's name in the messages.
static inline int dec_pack_tree(const char* who, int nlevels, const int* C, const hrseg_decode_tree_t* tree, unsigned* node,
                                int* Cout) {
  HRSEG_CHECK_ARG(nlevels >= 1 && nlevels <= HRSEG_DECODE_MAX_LEVELS, "%s: nlevels=%d not in 1..%d", who, nlevels,
                  HRSEG_DECODE_MAX_LEVELS);
  int total = 0;
  for (int L = 0; L < HRSEG_DECODE_MAX_LEVELS; ++L) Cout[L] = 0;
  for (int i = 0; i < DEC_NODES; ++i) node[i] = 0;
  for (int L = 0; L < nlevels; ++L) {
    HRSEG_CHECK_ARG(C[L] >= 1 && C[L] <= HRSEG_DECODE_MAX_CHANNELS, "%s: C[%d]=%d not in 1..%d", who, L, C[L],
                    HRSEG_DECODE_MAX_CHANNELS);
    Cout[L] = C[L];
    total += C[L];
  }
  HRSEG_CHECK_ARG(total <= 64, "%s: %d channels over all levels, at most 64", who, total);
  for (int L = 0; L < nlevels; ++L)
    for (int c = 0; c < C[L]; ++c) {
      const int first = tree->first_child[L][c], kids = tree->n_children[L][c], pv = tree->pixel_val[L][c];
      if (kids == 0) {
        HRSEG_CHECK_ARG(pv >= 0 && pv <= 255, "%s: leaf (level %d, channel %d) has pixel value %d", who, L, c, pv);
        node[L * HRSEG_DECODE_MAX_CHANNELS + c] = (unsigned)pv << 16;
      } else {
        HRSEG_CHECK_ARG(L + 1 < nlevels && kids > 0 && first >= 0 && first + kids <= C[L + 1],
                        "%s: children [%d, %d) of (level %d, channel %d) are not channels of the next level", who, first,
                        first + kids, L, c);
        node[L * HRSEG_DECODE_MAX_CHANNELS + c] = (unsigned)first | ((unsigned)kids << 8);
      }
    }
  return 0;
}

// every sample gets the same number of striding blocks (its size is known on the device only): about 8192 in all
static inline int dec_blocks_per_sample(int B) {
  const int per_sample = 8192 / B;
  return per_sample < 1 ? 1 : (per_sample > 1024 ? 1024 : per_sample);
}

// ---- the prelude and the launch that hrseg_decode_labels, hrseg_decode_views and hrseg_decode_windows share (host)
// the alignment the dword / float4 stores of the outputs need, then the tree (dec_pack_tree) and its root_softmax as 0 / 1
static inline int dec_outputs_and_tree(const char* who, int nlevels, const int* C, const hrseg_decode_tree_t* tree,
                                       const unsigned char* labels, const float* confidence, unsigned* node, int* Cout,
                                       int* root_softmax) {
  HRSEG_CHECK_ARG(((uintptr_t)labels & 3) == 0 && ((uintptr_t)confidence & 15) == 0,
                  "%s: labels must be 4-byte and confidence 16-byte aligned", who);
  if (const int rc = dec_pack_tree(who, nlevels, C, tree, node, Cout)) return rc;
  *root_softmax = tree->root_softmax ? 1 : 0;
  return 0;
}

// one set of level pointers z[0 .. nlevels) -> out[HRSEG_DECODE_MAX_LEVELS] (nullptr beyond nlevels)
static inline int dec_level_pointers(const char* who, int nlevels, const float* const* z, const float** out) {
  for (int L = 0; L < HRSEG_DECODE_MAX_LEVELS; ++L) {
    HRSEG_CHECK_ARG(L >= nlevels || z[L], "%s: level %d has no logits", who, L);
    out[L] = L < nlevels ? z[L] : nullptr;
  }
  return 0;
}

// the grid every decode uses, and the instantiation with or without the confidence
template <typename... P, typename... A>
static inline void dec_launch(void (*with_conf)(P...), void (*labels_only)(P...), const float* confidence, int B,
                              hrseg_stream_t stream, A... args) {
  const dim3 grid((unsigned)dec_blocks_per_sample(B), (unsigned)B);
  hipLaunchKernelGGL(confidence ? with_conf : labels_only, grid, dim3(DEC_TPB), 0, (hipStream_t)stream, args...);
}
