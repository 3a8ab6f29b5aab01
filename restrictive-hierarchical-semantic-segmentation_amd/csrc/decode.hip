// Device output pipeline: per-level logits at network size -> one uint8 label map per source image, at the source's own
// (ragged) size, in the pixel values of class_map.csv; optionally the confidence of the decoded path.  The semantics
// are stated in include/hrseg.h (hrseg_decode_labels): bilinear resample of the logits (torch align_corners=False),
// arg-max over the level-0 channels, then top-down through the tree: at every level only the child group of the node
// chosen above it competes, so the decoded path is always a path of the tree.
//
// One launch (family "decode_labels"), grid (blocks, B).  The output sizes live in the DEVICE descriptor table only, so
// the host cannot size a grid per sample: every sample gets the same number of blocks, which stride over the sample's
// tiles (blocks of a small sample run out of tiles at once).  A tile is 4 output rows x 256 pixels: one wave per row,
// one lane per 4 consecutive pixels.  The 4 pixels are cut at 4-byte boundaries of the packed label buffer (rows of a
// ragged buffer start at any byte), so an interior lane writes one full dword of labels and one float4 of confidences;
// only the lanes on a row's two edges fall back to byte stores.  The row taps and weights are computed once per lane,
// the column taps once per pixel.
//
// Only the channels of the groups on the decoded path are fetched (tl tree: 4 level-0 channels everywhere, the 4
// tooth channels only where "tooth" won), 4 taps each, through the vector cache: at 620 -> 1400x2900 an output row reuses
// its two source rows ~4.7 times along x and the next output rows reuse them again.  The design expects most taps to
// hit in cache for that reason; the hit rates and the HBM traffic have NOT been measured (no counter run was made), and
// neither has the alternative of fetching every channel.  The walk keeps no per-channel array:
// arg-max and (when the confidence is wanted) the soft-max denominator are carried online, so the group width (<= 16)
// costs no registers.
//
// The tree (<= 8 levels x 16 channels, one packed dword per node) and the level pointers are kernel arguments; the
// block copies the node table to LDS once because lanes index it with their own channel.
#include "decode_common.h"

struct DecodeArgs {
  const float* z[HRSEG_DECODE_MAX_LEVELS];
  int C[HRSEG_DECODE_MAX_LEVELS];
  unsigned node[DEC_NODES];                       // one packed dword per node (decode_common.h)
  int nlevels, root_softmax;
};

template <bool CONF>
__global__ __launch_bounds__(DEC_TPB) void decode_labels_kernel(DecodeArgs a, const long long* __restrict__ desc,
                                                                u8* __restrict__ labels, float* __restrict__ conf, int S) {
  __shared__ unsigned tab[DEC_NODES];
  if (threadIdx.x < DEC_NODES) tab[threadIdx.x] = a.node[threadIdx.x];
  __syncthreads();
  const int b = blockIdx.y, wave = threadIdx.x / HRSEG_WAVE, lane = threadIdx.x & (HRSEG_WAVE - 1);
  const long long off = desc[4 * b], H = desc[4 * b + 1], W = desc[4 * b + 2];
  if (H < 1 || W < 1) return;
  // a row may start at any byte: up to 3 pixels of padding in front of it, so (W + 3) pixels cover every alignment
  const long long tiles_x = (W + 3 + DEC_TILE_W - 1) / DEC_TILE_W, tiles_y = (H + DEC_ROWS - 1) / DEC_ROWS;
  const long long ntiles = tiles_x * tiles_y;
  const float sy = (float)S / (float)H, sx = (float)S / (float)W;
  const size_t plane = (size_t)S * S;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long ty = t / tiles_x, tx = t - ty * tiles_x;
    const long long y = ty * DEC_ROWS + wave;
    if (y >= H) continue;
    const long long row = off + y * W;                                    // first byte of the output row
    const int mis = (int)(((unsigned long long)(uintptr_t)labels + (unsigned long long)row) & 3ull);
    const long long x0 = (tx * HRSEG_WAVE + lane) * DEC_PX - mis;          // labels + row + x0 is 4-byte aligned
    if (x0 >= W || x0 + DEC_PX <= 0) continue;
    const DecLin ly = dec_lin((int)y, sy, S);
    const int r0 = ly.i0 * S, r1 = ly.i1 * S;

    DecLin lx[DEC_PX];
    int start[DEC_PX], n[DEC_PX];
    bool act[DEC_PX];
    unsigned pix[DEC_PX];
    float cf[DEC_PX];
#pragma unroll
    for (int p = 0; p < DEC_PX; ++p) {
      const long long x = x0 + p;
      act[p] = x >= 0 && x < W;
      lx[p] = dec_lin(act[p] ? (int)x : 0, sx, S);
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
      const float* __restrict__ zb = a.z[L] + (size_t)b * a.C[L] * plane;
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
#pragma unroll
        for (int p = 0; p < DEC_PX; ++p) {
          if (act[p] && k < n[p]) {
            const float* __restrict__ zc = zb + (size_t)(start[p] + k) * plane;
            const float p00 = zc[r0 + lx[p].i0], p01 = zc[r0 + lx[p].i1];
            const float p10 = zc[r1 + lx[p].i0], p11 = zc[r1 + lx[p].i1];
            const float t0 = __fadd_rn(__fmul_rn(p00, lx[p].l0), __fmul_rn(p01, lx[p].l1));
            const float t1 = __fadd_rn(__fmul_rn(p10, lx[p].l0), __fmul_rn(p11, lx[p].l1));
            const float v = __fadd_rn(__fmul_rn(t0, ly.l0), __fmul_rn(t1, ly.l1));
            if (v > best[p]) {                                // strict: the lowest index wins ties (torch.argmax)
              if (want_sum) sum[p] = sum[p] * expf(best[p] - v) + 1.f;
              best[p] = v;
              arg[p] = k;
            } else if (want_sum) {
              sum[p] += v == best[p] ? 1.f : expf(v - best[p]);   // equal also covers -inf against -inf (no NaN)
            }
          }
        }
      }
#pragma unroll
      for (int p = 0; p < DEC_PX; ++p) {
        if (!act[p]) continue;
        if (CONF) cf[p] *= want_sum ? 1.f / sum[p] : 1.f / (1.f + expf(-best[p]));
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

// ------------------------------------------------------------------------------------------------------------ C ABI
extern "C" int hrseg_decode_labels(int nlevels, const float* const* z, const int* C, const hrseg_decode_tree_t* tree,
                                   const long* desc, unsigned char* labels, float* confidence, int B, int S,
                                   hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(z && C && tree && desc && labels && B > 0 && B <= 65535 && S > 0 && S <= 32768,
                  "hrseg_decode_labels: bad arguments");
  DecodeArgs a;
  if (const int rc = dec_outputs_and_tree("hrseg_decode_labels", nlevels, C, tree, labels, confidence, a.node, a.C, &a.root_softmax))
    return rc;
  if (const int rc = dec_level_pointers("hrseg_decode_labels", nlevels, z, a.z)) return rc;
  a.nlevels = nlevels;
  dec_launch(decode_labels_kernel<true>, decode_labels_kernel<false>, confidence, B, stream, a, (const long long*)desc, labels,
             confidence, S);
  HRSEG_LAUNCH_CHECK("decode_labels");
  hrseg_count(CNT_DECODE_LABELS);
  return 0;
}
