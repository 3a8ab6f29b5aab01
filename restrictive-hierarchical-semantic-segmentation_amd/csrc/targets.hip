// The label-side plane builders, each with a 64-entry table as kernel argument: target encoding (label image -> the per-node
// target planes of the losses and metrics) and level synthesis for flat models.  gfx950.
#include "common.h"
#include "level_common.h"
#include "target_encode.h"

// --------------------------------------------------------------------------- target encoding
// Label image (one pixel value per leaf class) -> the per-node target planes the losses and
// metrics consume: SegDataset.separate_masks / traverse_tree / process_ignore_values of the reference
// (Data/dataset.py:41-124, 227-265) for an identity spatial transform.  on_lut[v] has bit c set when
// channel c's node contains the leaf whose pixel value is v (a parent = OR of its leaves), so one
// 8-byte table read per pixel replaces the per-node mask images.  HBM-bound: 1 byte in, 4*C out.
// Partial labels (PARTIAL): a second table, unk_lut[v], names the channels a pixel of value v says nothing about (the
// strict descendants of an internal node's byte, every channel for an ignore byte); the rule is encode_write's.
template <bool PARTIAL>
__global__ __launch_bounds__(256) void encode_targets_kernel(const unsigned char* __restrict__ label,
                                                             const unsigned long long* __restrict__ on_lut,
                                                             const unsigned long long* __restrict__ unk_lut,
                                                             TargetParents pr, float* __restrict__ out, int C, long hw,
                                                             long n) {
  __shared__ unsigned long long lut[256];
  __shared__ unsigned long long ulut[PARTIAL ? 256 : 1];
  lut[threadIdx.x] = on_lut[threadIdx.x];
  if constexpr (PARTIAL) ulut[threadIdx.x] = unk_lut[threadIdx.x];
  __syncthreads();
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long b = i / hw, pix = i - b * hw;
    const unsigned char v = label[i];
    encode_write(lut[v], PARTIAL ? ulut[v] : 0ull, pr, out + (size_t)b * C * hw + pix, C, (size_t)hw);
  }
}

// both entry points: `name` is the one that was called
static int encode_targets(const char* name, const unsigned char* label, const unsigned long long* on_lut,
                          const unsigned long long* unk_lut, bool partial, const int* parent, float* out, int B, int C,
                          long hw, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(label && on_lut && (!partial || unk_lut) && parent && out && B > 0 && hw > 0, "%s: bad arguments", name);
  HRSEG_CHECK_ARG(C >= 1 && C <= 64, "%s: C=%d not in 1..64", name, C);
  TargetParents pr;
  const int bad = target_parents(parent, C, pr);
  HRSEG_CHECK_ARG(bad < 0, "%s: parent[%d]=%d out of range", name, bad, parent[bad < 0 ? 0 : bad]);
  const long n = (long)B * hw;
  const dim3 grid(pixel_blocks(n, 8192));
  if (partial)
    hipLaunchKernelGGL(encode_targets_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, label, on_lut, unk_lut, pr, out, C,
                       hw, n);
  else
    hipLaunchKernelGGL(encode_targets_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, label, on_lut, unk_lut, pr, out, C,
                       hw, n);
  HRSEG_LAUNCH_CHECK(partial ? "encode_targets_partial" : "encode_targets");
  return 0;
}

extern "C" int hrseg_encode_targets(const unsigned char* label, const unsigned long long* on_lut, const int* parent,
                                    float* out, int B, int C, long hw, hrseg_stream_t stream) {
  return encode_targets("hrseg_encode_targets", label, on_lut, nullptr, false, parent, out, B, C, hw, stream);
}

extern "C" int hrseg_encode_targets_partial(const unsigned char* label, const unsigned long long* on_lut,
                                            const unsigned long long* unk_lut, const int* parent, float* out, int B, int C,
                                            long hw, hrseg_stream_t stream) {
  return encode_targets("hrseg_encode_targets_partial", label, on_lut, unk_lut, true, parent, out, B, C, hw, stream);
}

// --------------------------------------------------------------------------- level synthesis for flat models
// predictEval.py:85-185 (get_parent_masks / combine_levels): out[b][o][pix] is, per output channel o, either the COPY
// of one input channel (mask with a single bit) or the UNION "any selected channel > 0" (1.0 / 0.0) of the input
// channels whose bits are set.  Input channel i < C0 is plane i of x0, else plane i - C0 of x1 (the leaves and the
// already synthesised parents of combine_levels).  One thread per pixel, planes coalesced.
struct LevelTable { unsigned long long mask[64]; int is_union[64]; };
__global__ __launch_bounds__(256) void combine_levels_kernel(const float* __restrict__ x0, int C0,
                                                             const float* __restrict__ x1, int C1,
                                                             float* __restrict__ out, int Cout, long hw, long n,
                                                             LevelTable tab) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long b = i / hw, pix = i - b * hw;
    for (int o = 0; o < Cout; ++o) {
      unsigned long long m = tab.mask[o];
      float v = 0.f;
      while (m) {
        const int c = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float xv = (c < C0) ? x0[((size_t)b * C0 + c) * hw + pix] : x1[((size_t)b * C1 + (c - C0)) * hw + pix];
        if (tab.is_union[o]) v = (xv > 0.f) ? 1.f : v;
        else v = xv;
      }
      out[((size_t)b * Cout + o) * hw + pix] = v;
    }
  }
}

extern "C" int hrseg_combine_levels(const float* x0, int C0, const float* x1, int C1, const unsigned long long* masks,
                                    const int* is_union, float* out, int B, int Cout, long hw, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(x0 && masks && is_union && out && B > 0 && hw > 0 && C0 > 0 && C1 >= 0 && C0 + C1 <= 64 && Cout > 0 && Cout <= 64 &&
                      (C1 == 0 || x1), "hrseg_combine_levels: bad arguments (C0=%d C1=%d Cout=%d)", C0, C1, Cout);
  LevelTable tab;
  for (int o = 0; o < Cout; ++o) {
    HRSEG_CHECK_ARG(masks[o] != 0 && (C0 + C1 == 64 || (masks[o] >> (C0 + C1)) == 0),
                    "hrseg_combine_levels: channel %d selects no input / an input beyond %d", o, C0 + C1);
    tab.mask[o] = masks[o];
    tab.is_union[o] = is_union[o];
  }
  const long n = (long)B * hw;
  hipLaunchKernelGGL(combine_levels_kernel, dim3(pixel_blocks(n, 4096)), dim3(256), 0, (hipStream_t)stream, x0, C0, x1, C1, out, Cout,
                     hw, n, tab);
  HRSEG_LAUNCH_CHECK("combine_levels");
  return 0;
}
