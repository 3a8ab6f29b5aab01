// Hedged decode: the restrictive top-down decode of decode.hip that may end ABOVE a leaf.  The walk carries the composed
// confidence T_L of its path; entering node (L, c) needs T_L >= tau[L][c], otherwise the pixel is labelled with the byte of
// the node it stands on (its parent), or with reject_val where level 0 itself fails.  The semantics are stated in
// include/hrseg.h (hrseg_decode_hedged); with all-zero thresholds the labels and the confidence are those of
// hrseg_decode_labels bit for bit, because the resampling, the channel step and the confidence product below are the
// expressions of decode_labels_kernel, compiled with the same flags.
//
// One launch (family "decode_hedged"), the grid, the 4 x 256 tile, the handling of misaligned rows and the dword / float4
// stores of decode_labels_kernel (decode.hip describes them).  What differs:
//   * the soft-max denominator is always carried (the test needs T_L whether or not the confidence is stored); the
//     kernel is templated only on whether the confidence is stored;
//   * a lane whose 4 pixels lie outside the row does not leave the tile early: it stays, inactive, so that whole waves
//     reach the counting below;
//   * one packed dword per node holds the byte written when the walk ends ON the node -- a leaf's pixel value or an
//     internal node's stop value -- so a pixel keeps (byte, counter cell, confidence) of the node it stands on and a
//     failed test simply stops updating them;
//   * counters: sum C + 2 32-bit cells per block in LDS (a block counts pixels of one image, H*W <= 2^31).  Confident
//     background sends most lanes of a wave to one cell, so a lane whose 4 pixels share a cell adds 4 once, and equal
//     cells of a wave are folded before the LDS atomic (lm_wave_add, labelmap_common.h).  At the block's end the
//     non-zero cells go to the int64 table with one 64-bit vector atomic each.  Integer sums: the same bytes in every
//     run, whatever the block order, so there is no deterministic variant.
//
// The node table, the thresholds and the level pointers are kernel arguments (about 1.2 KiB); the block copies the two
// tables to LDS once because lanes index them with their own channel.
#include "decode_common.h"

#define HDG_MAX_CELLS (64 + 2)                      // sum C <= 64 tree nodes, then "rejected" and "nonfinite"

struct HedgeArgs {
  const float* z[HRSEG_DECODE_MAX_LEVELS];
  int C[HRSEG_DECODE_MAX_LEVELS];
  int cell0[HRSEG_DECODE_MAX_LEVELS];             // counter cell of channel 0 of level L (breadth-first channel order)
  unsigned node[DEC_NODES];                       // decode_common.h's dword; bits 16-23 also hold an internal node's stop value
  float tau[DEC_NODES];
  int nlevels, nodes, reject_val;                 // nodes = sum C: cell `nodes` is "rejected", `nodes + 1` "nonfinite"
};

template <bool CONF>
__global__ __launch_bounds__(DEC_TPB) void decode_hedged_kernel(HedgeArgs a, const long long* __restrict__ desc,
                                                                u8* __restrict__ labels, float* __restrict__ conf,
                                                                u64* __restrict__ stops, int S) {
  __shared__ unsigned tab[DEC_NODES];
  __shared__ float tau[DEC_NODES];
  __shared__ unsigned cells[HDG_MAX_CELLS];
  if (threadIdx.x < DEC_NODES) {
    tab[threadIdx.x] = a.node[threadIdx.x];
    tau[threadIdx.x] = a.tau[threadIdx.x];
  }
  if (threadIdx.x < HDG_MAX_CELLS) cells[threadIdx.x] = 0;
  __syncthreads();
  const int b = blockIdx.y, wave = threadIdx.x / HRSEG_WAVE, lane = threadIdx.x & (HRSEG_WAVE - 1);
  const long long off = desc[4 * b], H = desc[4 * b + 1], W = desc[4 * b + 2];
  if (H < 1 || W < 1) return;
  if (H > (1ll << 31) / W) return;                                        // H*W > 2^31: the 32-bit block counts could wrap
  // a row may start at any byte: up to 3 pixels of padding in front of it, so (W + 3) pixels cover every alignment
  const long long tiles_x = (W + 3 + DEC_TILE_W - 1) / DEC_TILE_W, tiles_y = (H + DEC_ROWS - 1) / DEC_ROWS;
  const long long ntiles = tiles_x * tiles_y;
  const float sy = (float)S / (float)H, sx = (float)S / (float)W;
  const size_t plane = (size_t)S * S;
  const int ncells = a.nodes + 2;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long ty = t / tiles_x, tx = t - ty * tiles_x;
    const long long y = ty * DEC_ROWS + wave;
    if (y >= H) continue;                                                 // (the whole wave: a wave is a row)
    const long long row = off + y * W;                                    // first byte of the output row
    const int mis = (int)(((unsigned long long)(uintptr_t)labels + (unsigned long long)row) & 3ull);
    const long long x0 = (tx * HRSEG_WAVE + lane) * DEC_PX - mis;          // labels + row + x0 is 4-byte aligned
    const DecLin ly = dec_lin((int)y, sy, S);
    const int r0 = ly.i0 * S, r1 = ly.i1 * S;

    DecLin lx[DEC_PX];
    int start[DEC_PX], n[DEC_PX], cell[DEC_PX];
    bool act[DEC_PX], in[DEC_PX];
    unsigned pix[DEC_PX];
    float cf[DEC_PX];
#pragma unroll
    for (int p = 0; p < DEC_PX; ++p) {
      const long long x = x0 + p;
      in[p] = act[p] = x >= 0 && x < W;                                   // a lane outside the row: four inactive pixels
      lx[p] = dec_lin(act[p] ? (int)x : 0, sx, S);
      start[p] = 0;
      n[p] = a.C[0];
      pix[p] = 0;
      cell[p] = 0;
      cf[p] = 1.f;
    }
    const bool full = in[0] && in[DEC_PX - 1];
    const bool some = in[0] || in[1] || in[2] || in[3];                   // (a row narrower than a lane may hold only the middle ones)

    for (int L = 0; L < a.nlevels; ++L) {
      int kmax = 0;
#pragma unroll
      for (int p = 0; p < DEC_PX; ++p) kmax = max(kmax, act[p] ? n[p] : 0);
      if (kmax == 0) break;
      const float* __restrict__ zb = a.z[L] + (size_t)b * a.C[L] * plane;
      const bool want_sum = L > 0;                                   // level 0 of a tree model is a sigmoid: no denominator
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
        const int c = start[p] + arg[p];
        float T = cf[p];
        T *= want_sum ? 1.f / sum[p] : 1.f / (1.f + expf(-best[p]));
        if (T < tau[L * HRSEG_DECODE_MAX_CHANNELS + c]) {             // (false for a NaN: it walks on, as the plain decode)
          if (L == 0) {
            pix[p] = (unsigned)a.reject_val & 0xffu;
            cell[p] = a.nodes;
            cf[p] = T;
          }                                                           // L >= 1: byte, cell and confidence of the parent stay
          act[p] = false;
          continue;
        }
        const unsigned e = tab[L * HRSEG_DECODE_MAX_CHANNELS + c];
        const int kids = (int)((e >> 8) & 0xffu);
        pix[p] = (e >> 16) & 0xffu;
        cell[p] = a.cell0[L] + c;
        cf[p] = T;
        if (kids == 0) {
          act[p] = false;
        } else {
          start[p] = (int)(e & 0xffu);
          n[p] = kids;
        }
      }
    }

    if (some) {
      u8* __restrict__ o = labels + row + x0;
      if (full) {
        *reinterpret_cast<unsigned*>(o) = pix[0] | (pix[1] << 8) | (pix[2] << 16) | (pix[3] << 24);
        if (CONF) *reinterpret_cast<f32x4*>(conf + row + x0) = f32x4{cf[0], cf[1], cf[2], cf[3]};
      } else {
#pragma unroll
        for (int p = 0; p < DEC_PX; ++p) {
          if (in[p]) {
            o[p] = (u8)pix[p];
            if (CONF) conf[row + x0 + p] = cf[p];
          }
        }
      }
    }

    if (stops) {                                                          // whole waves from here on
      const bool one = full && cell[1] == cell[0] && cell[2] == cell[0] && cell[3] == cell[0];
      lm_wave_add(cells, (unsigned)cell[0], DEC_PX, one, lane);
      if (__ballot(!one && some) != 0) {
#pragma unroll
        for (int p = 0; p < DEC_PX; ++p) lm_wave_add(cells, (unsigned)cell[p], 1, !one && in[p], lane);
      }
      bool bad[DEC_PX];
      bool any = false;
#pragma unroll
      for (int p = 0; p < DEC_PX; ++p) {
        bad[p] = in[p] && cf[p] != cf[p];
        any = any || bad[p];
      }
      if (__ballot(any) != 0) {
#pragma unroll
        for (int p = 0; p < DEC_PX; ++p) lm_wave_add(cells, (unsigned)(a.nodes + 1), 1, bad[p], lane);
      }
    }
  }
  if (!stops) return;
  __syncthreads();
  if ((int)threadIdx.x < ncells && cells[threadIdx.x])
    atomicAdd(&stops[(size_t)b * ncells + threadIdx.x], (u64)cells[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------------------ C ABI
extern "C" int hrseg_decode_hedged(int nlevels, const float* const* z, const int* C, const hrseg_decode_tree_t* tree,
                                   const hrseg_hedge_t* hedge, const long* desc, unsigned char* labels, float* confidence,
                                   long long* stops, int B, int S, hrseg_stream_t stream) {
  const char* who = "hrseg_decode_hedged";
  HRSEG_CHECK_ARG(z && C && tree && hedge && desc && labels && B > 0 && B <= 65535 && S > 0 && S <= 32768,
                  "hrseg_decode_hedged: bad arguments");
  HedgeArgs a;
  int root_softmax = 0;
  if (const int rc = dec_outputs_and_tree(who, nlevels, C, tree, labels, confidence, a.node, a.C, &root_softmax)) return rc;
  HRSEG_CHECK_ARG(!root_softmax, "%s: root_softmax is set: a flat model has no path to shorten", who);
  HRSEG_CHECK_ARG(hedge->reject_val >= -1 && hedge->reject_val <= 255, "%s: reject_val=%d not in -1..255", who, hedge->reject_val);
  int owner[256];                                   // 1 + L * 16 + c of the node that writes the byte, 1 + DEC_NODES: reject_val
  for (int v = 0; v < 256; ++v) owner[v] = 0;
  if (hedge->reject_val >= 0) owner[hedge->reject_val] = 1 + DEC_NODES;
  a.nodes = 0;
  for (int i = 0; i < DEC_NODES; ++i) a.tau[i] = 0.f;
  for (int L = 0; L < HRSEG_DECODE_MAX_LEVELS; ++L) a.cell0[L] = 0;
  for (int L = 0; L < nlevels; ++L) {
    a.cell0[L] = a.nodes;
    a.nodes += C[L];
    for (int c = 0; c < C[L]; ++c) {
      const float t = hedge->tau[L][c];
      HRSEG_CHECK_ARG(t >= 0.f && t <= 1.f, "%s: tau of (level %d, channel %d) is %g, not in 0..1", who, L, c, (double)t);
      HRSEG_CHECK_ARG(L > 0 || t == 0.f || hedge->reject_val >= 0,
                      "%s: reject_val=-1 (no rejection), but (level 0, channel %d) has the threshold %g", who, c, (double)t);
      a.tau[L * HRSEG_DECODE_MAX_CHANNELS + c] = t;
      const int i = L * HRSEG_DECODE_MAX_CHANNELS + c;
      int v = tree->pixel_val[L][c];
      if (tree->n_children[L][c] != 0) {
        v = hedge->stop_val[L][c];
        HRSEG_CHECK_ARG(v >= 0 && v <= 255, "%s: internal node (level %d, channel %d) has stop value %d", who, L, c, v);
        a.node[i] |= (unsigned)v << 16;
      }
      if (owner[v] == 1 + DEC_NODES) {
        HRSEG_CHECK_ARG(false, "%s: (level %d, channel %d) and reject_val share the byte %d", who, L, c, v);
      }
      HRSEG_CHECK_ARG(owner[v] == 0, "%s: (level %d, channel %d) and (level %d, channel %d) share the byte %d", who,
                      (owner[v] - 1) / HRSEG_DECODE_MAX_CHANNELS, (owner[v] - 1) % HRSEG_DECODE_MAX_CHANNELS, L, c, v);
      owner[v] = 1 + i;
    }
  }
  HRSEG_CHECK_ARG(((uintptr_t)stops & 7) == 0, "%s: stops must be 8-byte aligned", who);
  if (const int rc = dec_level_pointers(who, nlevels, z, a.z)) return rc;
  a.nlevels = nlevels;
  a.reject_val = hedge->reject_val;
  dec_launch(decode_hedged_kernel<true>, decode_hedged_kernel<false>, confidence, B, stream, a, (const long long*)desc, labels,
             confidence, (u64*)stops, S);
  HRSEG_LAUNCH_CHECK("decode_hedged");
  hrseg_count(CNT_DECODE_HEDGED);
  return 0;
}
