// Test-time augmentation of the device output pipeline: hrseg_decode_views decodes the MEAN logit of up to 8 views (the
// network's logits for mirrored and/or rescaled copies of one batch) straight to source-size label maps, and
// hrseg_flip_views builds the mirrored network inputs of one scale.  Semantics: include/hrseg.h.
//
// decode_views_kernel keeps the tile shape of decode_labels_kernel (decode.hip): grid (blocks, B), striding blocks per
// sample, a tile of 4 output rows x 256 pixels, one wave per row, one lane per 4 pixels cut at 4-byte boundaries of the
// packed label buffer, byte stores only on a row's two edges, node table in LDS.  One launch (family "decode_views"), no
// workspace: the V x L level pointers, the view sizes and the flip flags travel as kernel arguments.
//
// The restrictive decode needs the mean logit of the channels on the decoded path only, so per channel step a lane
// fetches V x 4 taps for each of its 4 pixels and nothing else; arg-max and the soft-max denominator are carried online
// over the mean, exactly as the single-view kernel carries them over its one logit.
//
// Registers: the taps and weights of 4 columns and 1 row are 20 registers, the same as in the single-view kernel, and
// eight such sets do not fit beside the walk.  The kernel holds ONE set, that of the view size it used last: a flipped
// view of the same size shares the unflipped view's taps (it reads source index S - 1 - i with the same weights), so a
// flip-only ensemble computes its taps once per tile and a multi-scale ensemble recomputes them where consecutive views
// differ in size (a wave-uniform branch).  The per-view resampling scales S_v / H_b and S_v / W_b are computed once per
// block into LDS.
#include "decode_common.h"

// The float arithmetic of a channel step, spelled with the fused multiply-adds the compiler makes of decode_labels_kernel's
// expressions and with its own contraction switched off in this unit: whatever the optimiser does around a call (it
// peels the first view off the view loop), every view's logit rounds as the single-view kernel rounds its one logit, so
// one unflipped view is hrseg_decode_labels bit for bit and flipped copies of one logit set are too (tests/test_decode_views_gpu.py).
#pragma clang fp contract(off)

#define DEC_VIEWS HRSEG_DECODE_MAX_VIEWS

struct DecodeViewsArgs {
  const float* z[DEC_VIEWS * HRSEG_DECODE_MAX_LEVELS];     // view-major: z[v * HRSEG_DECODE_MAX_LEVELS + L]
  int C[HRSEG_DECODE_MAX_LEVELS];
  unsigned node[DEC_NODES];                                // one packed dword per node (decode_common.h)
  int S[DEC_VIEWS], flags[DEC_VIEWS];
  int nviews, nlevels, root_softmax;
  float inv_views;                                         // 1.0f / nviews
};

template <bool CONF>
__global__ __launch_bounds__(DEC_TPB) void decode_views_kernel(DecodeViewsArgs a, const long long* __restrict__ desc,
                                                               u8* __restrict__ labels, float* __restrict__ conf) {
  __shared__ unsigned tab[DEC_NODES];
  __shared__ float scale_y[DEC_VIEWS], scale_x[DEC_VIEWS];
  const int b = blockIdx.y, wave = threadIdx.x / HRSEG_WAVE, lane = threadIdx.x & (HRSEG_WAVE - 1);
  const long long off = desc[4 * b], H = desc[4 * b + 1], W = desc[4 * b + 2];
  if (H < 1 || W < 1) return;
  if (threadIdx.x < DEC_NODES) tab[threadIdx.x] = a.node[threadIdx.x];
  if (threadIdx.x < a.nviews) {
    scale_y[threadIdx.x] = (float)a.S[threadIdx.x] / (float)H;
    scale_x[threadIdx.x] = (float)a.S[threadIdx.x] / (float)W;
  }
  __syncthreads();
  // a row may start at any byte: up to 3 pixels of padding in front of it, so (W + 3) pixels cover every alignment
  const long long tiles_x = (W + 3 + DEC_TILE_W - 1) / DEC_TILE_W, tiles_y = (H + DEC_ROWS - 1) / DEC_ROWS;
  const long long ntiles = tiles_x * tiles_y;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long ty = t / tiles_x, tx = t - ty * tiles_x;
    const long long y = ty * DEC_ROWS + wave;
    if (y >= H) continue;
    const long long row = off + y * W;                                    // first byte of the output row
    const int mis = (int)(((unsigned long long)(uintptr_t)labels + (unsigned long long)row) & 3ull);
    const long long x0 = (tx * HRSEG_WAVE + lane) * DEC_PX - mis;          // labels + row + x0 is 4-byte aligned
    if (x0 >= W || x0 + DEC_PX <= 0) continue;

    int cur = a.S[0];                                                     // the view size whose taps are held
    DecLin ly = dec_lin((int)y, scale_y[0], cur);
    DecLin lx[DEC_PX];
    int start[DEC_PX], n[DEC_PX];
    bool act[DEC_PX];
    unsigned pix[DEC_PX];
    float cf[DEC_PX];
#pragma unroll
    for (int p = 0; p < DEC_PX; ++p) {
      const long long x = x0 + p;
      act[p] = x >= 0 && x < W;
      lx[p] = dec_lin(act[p] ? (int)x : 0, scale_x[0], cur);
      start[p] = 0;
      n[p] = a.C[0];
      pix[p] = 0;
      cf[p] = 1.f;
    }
    const bool full = act[0] && act[DEC_PX - 1];

    for (int L = 0; L < a.nlevels; ++L) {
      int kmax = 0;
#pragma unroll
      for (int p = 0; p < DEC_PX; ++p) kmax = max(kmax, act[p] ? n[p] : 0);
      if (kmax == 0) break;
      const size_t sample = (size_t)b * a.C[L];
      const bool want_sum = CONF && (L > 0 || a.root_softmax);     // level 0 of a tree model is a sigmoid: no denominator
      float best[DEC_PX], sum[DEC_PX];
      int arg[DEC_PX];
#pragma unroll
      for (int p = 0; p < DEC_PX; ++p) {
        best[p] = -INFINITY;
        sum[p] = 0.f;
        arg[p] = 0;
      }
      for (int k = 0; k < kmax; ++k) {
        float acc[DEC_PX];
#pragma unroll
        for (int p = 0; p < DEC_PX; ++p) acc[p] = 0.f;
        for (int v = 0; v < a.nviews; ++v) {
          const int S = a.S[v], fl = a.flags[v];
          if (S != cur) {                                          // wave-uniform: S is a kernel argument
            cur = S;
            ly = dec_lin((int)y, scale_y[v], S);
#pragma unroll
            for (int p = 0; p < DEC_PX; ++p) lx[p] = dec_lin((int)(x0 + p), scale_x[v], S);   // off the row: taps unused
          }
          const size_t plane = (size_t)S * S;
          const float* __restrict__ zb = a.z[v * HRSEG_DECODE_MAX_LEVELS + L] + sample * plane;
          const bool fx = fl & HRSEG_VIEW_HFLIP, fy = fl & HRSEG_VIEW_VFLIP;
          const int r0 = (fy ? S - 1 - ly.i0 : ly.i0) * S, r1 = (fy ? S - 1 - ly.i1 : ly.i1) * S;
#pragma unroll
          for (int p = 0; p < DEC_PX; ++p) {
            if (act[p] && k < n[p]) {
              const float* __restrict__ zc = zb + (size_t)(start[p] + k) * plane;
              const int c0 = fx ? S - 1 - lx[p].i0 : lx[p].i0, c1 = fx ? S - 1 - lx[p].i1 : lx[p].i1;
              const float p00 = zc[r0 + c0], p01 = zc[r0 + c1];
              const float p10 = zc[r1 + c0], p11 = zc[r1 + c1];
              const float r = dec_blend(p00, p01, p10, p11, lx[p].l0, lx[p].l1, ly.l0, ly.l1);
              acc[p] = v == 0 ? r : __fadd_rn(acc[p], r);          // in view order
            }
          }
        }
#pragma unroll
        for (int p = 0; p < DEC_PX; ++p) {
          if (act[p] && k < n[p]) {
            const float m = __fmul_rn(acc[p], a.inv_views);        // one view: r_0 * 1.0f = r_0
            dec_step(m, k, want_sum, best[p], sum[p], arg[p]);
          }
        }
      }
#pragma unroll
      for (int p = 0; p < DEC_PX; ++p) {
        if (!act[p]) continue;
        if (CONF) cf[p] *= dec_factor(want_sum, best[p], sum[p]);
        const unsigned e = tab[L * HRSEG_DECODE_MAX_CHANNELS + start[p] + arg[p]];
        const int kids = (int)((e >> 8) & 0xffu);
        if (kids == 0) {
          pix[p] = (e >> 16) & 0xffu;
          act[p] = false;
        } else {
          start[p] = (int)(e & 0xffu);
          n[p] = kids;
        }
      }
    }

    u8* __restrict__ o = labels + row + x0;
    if (full) {
      *reinterpret_cast<unsigned*>(o) = pix[0] | (pix[1] << 8) | (pix[2] << 16) | (pix[3] << 24);
      if (CONF) *reinterpret_cast<f32x4*>(conf + row + x0) = f32x4{cf[0], cf[1], cf[2], cf[3]};
    } else {
#pragma unroll
      for (int p = 0; p < DEC_PX; ++p) {
        const long long x = x0 + p;
        if (x >= 0 && x < W) {
          o[p] = (u8)pix[p];
          if (CONF) conf[row + x] = cf[p];
        }
      }
    }
  }
}

// out block v = x mirrored by flags[v] (2 bits per view in `packed`); one lane moves VEC consecutive floats of an output row
template <int VEC>
__global__ __launch_bounds__(256) void flip_views_kernel(const float* __restrict__ x, float* __restrict__ out, unsigned packed,
                                                         unsigned rows_per_view, unsigned H, unsigned Wv, unsigned total) {
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const unsigned r = i / Wv, q = i - r * Wv;                  // output row over all views, position in it
    const unsigned v = r / rows_per_view, rv = r - v * rows_per_view;
    const unsigned img = rv / H, y = rv - img * H;
    const unsigned fl = (packed >> (2 * v)) & 3u;
    const unsigned sy = (fl & HRSEG_VIEW_VFLIP) ? H - 1 - y : y, sq = (fl & HRSEG_VIEW_HFLIP) ? Wv - 1 - q : q;
    const size_t src = ((size_t)img * H + sy) * Wv + sq;
    if (VEC == 4) {
      const f32x4 s = reinterpret_cast<const f32x4*>(x)[src];
      reinterpret_cast<f32x4*>(out)[i] = (fl & HRSEG_VIEW_HFLIP) ? f32x4{s[3], s[2], s[1], s[0]} : s;
    } else {
      out[i] = x[src];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ C ABI
extern "C" int hrseg_decode_views(int nviews, const int* S, const int* flags, int nlevels, const float* const* z, const int* C,
                                  const hrseg_decode_tree_t* tree, const long* desc, unsigned char* labels, float* confidence,
                                  int B, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(nviews >= 1 && nviews <= HRSEG_DECODE_MAX_VIEWS, "hrseg_decode_views: nviews=%d not in 1..%d", nviews,
                  HRSEG_DECODE_MAX_VIEWS);
  HRSEG_CHECK_ARG(S && flags && z && C && tree && desc && labels && B > 0 && B <= 65535, "hrseg_decode_views: bad arguments");
  DecodeViewsArgs a = {};
  if (const int rc = dec_outputs_and_tree("hrseg_decode_views", nlevels, C, tree, labels, confidence, a.node, a.C, &a.root_softmax))
    return rc;
  for (int v = 0; v < nviews; ++v) {
    HRSEG_CHECK_ARG(S[v] >= 1 && S[v] <= 32768, "hrseg_decode_views: S[%d]=%d not in 1..32768", v, S[v]);
    HRSEG_CHECK_ARG(flags[v] >= 0 && flags[v] <= 3, "hrseg_decode_views: flags[%d]=%d not in 0..3", v, flags[v]);
    a.S[v] = S[v];
    a.flags[v] = flags[v];
    for (int L = 0; L < nlevels; ++L) {
      HRSEG_CHECK_ARG(z[v * nlevels + L], "hrseg_decode_views: view %d, level %d has no logits", v, L);
      a.z[v * HRSEG_DECODE_MAX_LEVELS + L] = z[v * nlevels + L];
    }
  }
  a.nviews = nviews;
  a.nlevels = nlevels;
  a.inv_views = 1.0f / (float)nviews;
  dec_launch(decode_views_kernel<true>, decode_views_kernel<false>, confidence, B, stream, a, (const long long*)desc, labels,
             confidence);
  HRSEG_LAUNCH_CHECK("decode_views");
  hrseg_count(CNT_DECODE_VIEWS);
  return 0;
}

extern "C" int hrseg_flip_views(const float* x, float* out, int nviews, const int* flags, int B, int C, int H, int W,
                                hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(nviews >= 1 && nviews <= HRSEG_DECODE_MAX_VIEWS, "hrseg_flip_views: nviews=%d not in 1..%d", nviews,
                  HRSEG_DECODE_MAX_VIEWS);
  HRSEG_CHECK_ARG(x && out && flags && B > 0 && C > 0 && H > 0 && W > 0, "hrseg_flip_views: bad arguments");
  unsigned packed = 0;
  for (int v = 0; v < nviews; ++v) {
    HRSEG_CHECK_ARG(flags[v] >= 0 && flags[v] <= 3, "hrseg_flip_views: flags[%d]=%d not in 0..3", v, flags[v]);
    packed |= (unsigned)flags[v] << (2 * v);
  }
  const long long rows_per_view = (long long)B * C * H, elems = rows_per_view * nviews * W;
  HRSEG_CHECK_ARG(elems < (1ll << 31), "hrseg_flip_views: %lld output elements, at most 2^31 - 1", elems);
  // float4 moves where every row is a whole number of 16-byte granules of both tensors
  const bool vec = (W & 3) == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
  const unsigned Wv = (unsigned)(vec ? W / 4 : W), total = (unsigned)(rows_per_view * nviews) * Wv;
  unsigned blocks = (total + 255u) / 256u;
  blocks = blocks > 4096u ? 4096u : blocks;
  if (vec)
    hipLaunchKernelGGL(flip_views_kernel<4>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, out, packed,
                       (unsigned)rows_per_view, (unsigned)H, Wv, total);
  else
    hipLaunchKernelGGL(flip_views_kernel<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, out, packed,
                       (unsigned)rows_per_view, (unsigned)H, Wv, total);
  HRSEG_LAUNCH_CHECK("flip_views");
  hrseg_count(CNT_FLIP_VIEWS);
  return 0;
}
