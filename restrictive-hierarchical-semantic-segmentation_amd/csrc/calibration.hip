// Device calibration scoring: per-level logits at network size + ground-truth label maps at the SOURCE size -> per tree
// node (and per level for the decoded path's "top label") a reliability histogram of integers: how often the model is right
// when it says p.  The semantics are stated in include/hrseg.h (hrseg_score_calibration): the logits are resampled with the
// decode's own multiplies and adds (decode.hip step 1), scaled by 1/T per level, composed down the tree exactly as the model
// composes them (P_child = P_parent * softmax_group(z)), and every (probability, outcome) event is quantised to 2^-24 and
// added to one cell of hist[img][row][bin][4] = (n, pos, sum_q, sum_e2).  Everything accumulated is an integer: the same
// bytes whatever the block order, so there is no deterministic variant.
//
// One launch (family "score_calibration"), grid (blocks, B) as the decode: the sizes live in the DEVICE descriptor table only,
// so every sample gets the same number of blocks, which stride over the sample's tiles; a block past the last tile leaves at
// once.  A tile is 4 output rows x 64 pixels: one wave per row, ONE pixel per lane (the decode's 4 do not fit: a level's 16
// logits, 16 scan temporaries and the 16 parent probabilities are live at once, 48 registers per pixel).  The row taps are
// computed once per lane and tile, the column taps once per pixel.
//
// Unlike the decode every group is fetched, and a level's probabilities stay alive while the next level is composed.  The
// tree is the same for every lane, so the walk is written with STATIC channel indices (loops over 16 fully unrolled, bounds
// and group edges wave-uniform values read from the kernel arguments): a group's maximum and denominator are two segmented
// scans (forward, then backward) over the level's 16 slots, which needs no per-lane indexing.  Only two things are indexed:
// the parent's probability (a uniform index, resolved by a select chain over the 16 slots) and the decoded path's node (the
// lane's own channel, looked up in the LDS copy of the node table as the decode does).
//
// The histogram is privatised per block in LDS, R x (n_bins + 1) cells of three 64-bit words (n | pos << 32, sum_q, sum_e2;
// a block counts pixels of one image, H*W <= 2^31, so n and pos fit 32 bits): 24 bytes per cell, sized per launch -- 3.8 KB for
// the tl tree at 15 bins, 57 KB at the limits (72 rows x 33 bins).  At the block's end the non-zero words go to the int64
// records with 64-bit vector atomics.  Real maps are dominated by confident background, so most lanes of a wave add to the
// same cell; the LDS atomic unit serialises them.  Folding equal cells inside the wave first (lm_wave_add, labelmap_common.h)
// has not been tried: the sums are 64-bit and differ per lane.
#include "decode_common.h"

#define CAL_TPB DEC_TPB
#define CAL_ROWS (CAL_TPB / HRSEG_WAVE)            // rows per tile: one per wave
#define CAL_TILE_W HRSEG_WAVE                     // one pixel per lane
#define CAL_CH HRSEG_DECODE_MAX_CHANNELS
#define CAL_ONE 16777216.f                        // 2^24: the probability grid
#define CAL_WORDS 3                               // 64-bit LDS words per cell

struct CalArgs {
  const float* z[HRSEG_DECODE_MAX_LEVELS];
  int C[HRSEG_DECODE_MAX_LEVELS];
  int row0[HRSEG_DECODE_MAX_LEVELS];              // first histogram row of level L's nodes
  float inv_temp[HRSEG_DECODE_MAX_LEVELS];
  unsigned node[DEC_NODES];                       // the decode's packed node (decode_common.h)
  unsigned up[DEC_NODES];                         // channel c of level L: first channel of its group | count << 8 | parent << 16
  int nlevels, root_softmax, n_bins, nodes, per_image;   // nodes = sum C: the top-label rows follow them
};

// one event (probability p, outcome y) into the block's cell of (row, bin): hrseg.h step 6
__device__ __forceinline__ void cal_event(u64* hist, int row, int n_bins, float p, bool y) {
  u64* cell = hist + (size_t)(row * (n_bins + 1)) * CAL_WORDS;
  const u64 one = 1ull | (y ? 1ull << 32 : 0ull);
  if (p != p) {                                   // before the clamp: fminf / fmaxf would swallow the NaN
    atomicAdd(cell + (size_t)n_bins * CAL_WORDS, one);
    return;
  }
  const unsigned q = (unsigned)rintf(__fmul_rn(fminf(fmaxf(p, 0.f), 1.f), CAL_ONE));
  const unsigned bin = min((unsigned)(n_bins - 1), (q * (unsigned)n_bins) >> 24);    // q <= 2^24, n_bins <= 32: 32 bits hold it
  const unsigned e = y ? 16777216u - q : q;
  const unsigned e12 = (e + 2048u) >> 12;
  cell += (size_t)bin * CAL_WORDS;
  atomicAdd(cell, one);
  atomicAdd(cell + 1, (u64)q);
  atomicAdd(cell + 2, (u64)(e12 * e12));
}

__global__ __launch_bounds__(CAL_TPB) void score_calibration_kernel(CalArgs a, const u8* __restrict__ gt,
                                                                    const long long* __restrict__ gdesc,
                                                                    const u64* __restrict__ path_lut, u64* __restrict__ out,
                                                                    u64* __restrict__ ignored, int S) {
  extern __shared__ u64 hist[];                   // [R * (n_bins + 1)][CAL_WORDS], then one word: the ignored pixels
  __shared__ unsigned tab[DEC_NODES];
  __shared__ u64 lut[256];
  const int b = blockIdx.y, tid = threadIdx.x, wave = tid / HRSEG_WAVE, lane = tid & (HRSEG_WAVE - 1);
  const long long off = gdesc[4 * b], H = gdesc[4 * b + 1], W = gdesc[4 * b + 2];
  if (H < 1 || W < 1 || off < 0) return;
  if (H > (1ll << 31) / W) return;                 // H*W > 2^31: the 32-bit halves of a block's counts could wrap
  const long long tiles_x = (W + CAL_TILE_W - 1) / CAL_TILE_W, tiles_y = (H + CAL_ROWS - 1) / CAL_ROWS;
  const long long ntiles = tiles_x * tiles_y;
  if ((long long)blockIdx.x >= ntiles) return;

  const int R = a.nodes + a.nlevels, cells = R * (a.n_bins + 1), words = cells * CAL_WORDS;
  for (int i = tid; i <= words; i += CAL_TPB) hist[i] = 0;
  if (tid < DEC_NODES) tab[tid] = a.node[tid];
  {
    u64 e = path_lut[tid];                         // CAL_TPB == 256: one table entry per thread
    LM_PATH_ENTRY(e, a)
    lut[tid] = e;
  }
  __syncthreads();

  const float sy = (float)S / (float)H, sx = (float)S / (float)W;
  const size_t plane = (size_t)S * S;
  const u8* __restrict__ gs = gt + off;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long ty = t / tiles_x, tx = t - ty * tiles_x;
    const long long y = ty * CAL_ROWS + wave, x = tx * CAL_TILE_W + lane;
    const bool inside = y < H && x < W;
    const u64 g = inside ? lut[gs[y * W + x]] : 0;
    const u64 skipped = __ballot(inside && g == 0);
    if (lane == 0 && skipped) atomicAdd(&hist[words], (u64)__popcll(skipped));
    if (g == 0) continue;
    const DecLin ly = dec_lin((int)y, sy, S), lx = dec_lin((int)x, sx, S);
    const int o00 = ly.i0 * S + lx.i0, o01 = ly.i0 * S + lx.i1, o10 = ly.i1 * S + lx.i0, o11 = ly.i1 * S + lx.i1;

    float pp[CAL_CH];                              // the level above: P of its channels
#pragma unroll
    for (int c = 0; c < CAL_CH; ++c) pp[c] = 1.f;
    bool alive = true;                             // the decoded path reaches this level
    int gfirst = 0, gcnt = a.C[0];                 // ... and its group there
    for (int L = 0; L < a.nlevels; ++L) {
      const int CL = a.C[L];
      const float* __restrict__ zb = a.z[L] + (size_t)b * CL * plane;
      const float it = a.inv_temp[L];
      const unsigned* __restrict__ up = a.up + L * CAL_CH;
      float v[CAL_CH], s[CAL_CH];
      // ---- the level's logits: four channels' taps in flight at once (a slot past the level re-reads its last channel)
#pragma unroll
      for (int c0 = 0; c0 < CAL_CH; c0 += 4) {
        if (c0 < CL) {
          float tp[4][4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float* __restrict__ zc = zb + (size_t)min(c0 + j, CL - 1) * plane;
            tp[j][0] = zc[o00];
            tp[j][1] = zc[o01];
            tp[j][2] = zc[o10];
            tp[j][3] = zc[o11];
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float t0 = __fadd_rn(__fmul_rn(tp[j][0], lx.l0), __fmul_rn(tp[j][1], lx.l1));
            const float t1 = __fadd_rn(__fmul_rn(tp[j][2], lx.l0), __fmul_rn(tp[j][3], lx.l1));
            v[c0 + j] = __fmul_rn(__fadd_rn(__fmul_rn(t0, ly.l0), __fmul_rn(t1, ly.l1)), it);
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[c0 + j] = -INFINITY;
        }
      }
      // ---- the decoded path: arg-max of the LOGITS over the group of the node chosen above (strict: lowest index wins)
      int arg = gfirst;
      {
        float best = -INFINITY;
#pragma unroll
        for (int c = 0; c < CAL_CH; ++c)
          if (c >= gfirst && c < gfirst + gcnt && v[c] > best) {
            best = v[c];
            arg = c;
          }
      }
      // ---- node probabilities
      if (L == 0 && !a.root_softmax) {
#pragma unroll
        for (int c = 0; c < CAL_CH; ++c) v[c] = 1.f / (1.f + expf(-v[c]));
      } else {
        // group maximum: a running maximum restarted at every group's first channel, then carried back from its last
        float run = -INFINITY;
#pragma unroll
        for (int c = 0; c < CAL_CH; ++c) {
          const bool first = (up[c] & 0xffu) == (unsigned)c;
          run = (first || v[c] > run) ? v[c] : run;
          s[c] = run;
        }
#pragma unroll
        for (int c = CAL_CH - 1; c >= 0; --c) {
          const bool last = (up[c] & 0xffu) + ((up[c] >> 8) & 0xffu) == (unsigned)(c + 1);
          run = last ? s[c] : run;
          s[c] = run;
        }
        // exponentials (equal also covers -inf against -inf) and the group's denominator, added in channel order
#pragma unroll
        for (int c = 0; c < CAL_CH; ++c) v[c] = v[c] == s[c] ? 1.f : expf(v[c] - s[c]);
#pragma unroll
        for (int c = 0; c < CAL_CH; ++c) {
          const bool first = (up[c] & 0xffu) == (unsigned)c;
          run = first ? v[c] : run + v[c];
          s[c] = run;
        }
#pragma unroll
        for (int c = CAL_CH - 1; c >= 0; --c) {
          const bool last = (up[c] & 0xffu) + ((up[c] >> 8) & 0xffu) == (unsigned)(c + 1);
          run = last ? s[c] : run;
          s[c] = run;
        }
#pragma unroll
        for (int c = 0; c < CAL_CH; ++c) {
          if (c < CL) {
            const unsigned par = up[c] >> 16;        // uniform: a select chain, no per-lane indexing
            float parent = pp[0];
#pragma unroll
            for (int k = 1; k < CAL_CH; ++k) parent = par == (unsigned)k ? pp[k] : parent;
            v[c] = parent * (v[c] / s[c]);
          }
        }
      }
      // ---- events: every node of the level, then the path's top label
      const int gl = (int)((g >> (8 * L)) & 0xffu) - 1;      // the ground truth's channel at this level, -1: none
      float top = 0.f;
#pragma unroll
      for (int c = 0; c < CAL_CH; ++c) {
        if (c < CL) cal_event(hist, a.row0[L] + c, a.n_bins, v[c], gl == c);
        top = c == arg ? v[c] : top;
        pp[c] = v[c];
      }
      if (alive && gl >= 0) cal_event(hist, a.nodes + L, a.n_bins, top, arg == gl);
      if (alive) {
        const unsigned e = tab[L * CAL_CH + arg];
        gcnt = (int)((e >> 8) & 0xffu);
        gfirst = (int)(e & 0xffu);
        if (gcnt == 0) alive = false;
      }
      if (!alive) gfirst = gcnt = 0;
    }
  }
  __syncthreads();

  // ---- flush: non-zero words -> the int64 records (n and pos unpacked)
  const size_t img = a.per_image ? (size_t)b : 0;
  u64* __restrict__ o = out + img * (size_t)cells * 4;
  for (int i = tid; i < words; i += CAL_TPB) {
    const u64 w = hist[i];
    if (w == 0) continue;
    const int cell = i / CAL_WORDS, k = i - cell * CAL_WORDS;
    if (k == 0) {
      atomicAdd(&o[cell * 4], w & 0xffffffffull);
      if (w >> 32) atomicAdd(&o[cell * 4 + 1], w >> 32);
    } else {
      atomicAdd(&o[cell * 4 + 1 + k], w);
    }
  }
  if (tid == 0 && hist[words]) atomicAdd(&ignored[img], hist[words]);
}

// ------------------------------------------------------------------------------------------------------------ C ABI
extern "C" int hrseg_score_calibration(int nlevels, const float* const* z, const int* C, const hrseg_decode_tree_t* tree,
                                       const float* inv_temp, const unsigned char* gt, const long* gdesc,
                                       const unsigned long long* path_lut, int n_bins, long long* hist, long long* ignored,
                                       int B, int S, int per_image, hrseg_stream_t stream) {
  static const char* who = "hrseg_score_calibration";
  HRSEG_CHECK_ARG(z && C && tree && inv_temp && gt && gdesc && path_lut && hist && ignored, "%s: null pointer", who);
  HRSEG_CHECK_ARG(B > 0 && B <= 65535, "%s: B=%d not in 1..65535", who, B);
  HRSEG_CHECK_ARG(S > 0 && S <= 32768, "%s: S=%d not in 1..32768", who, S);
  HRSEG_CHECK_ARG(n_bins >= 1 && n_bins <= HRSEG_CALIBRATION_MAX_BINS, "%s: n_bins=%d not in 1..%d", who, n_bins,
                  HRSEG_CALIBRATION_MAX_BINS);
  HRSEG_CHECK_ARG(((uintptr_t)hist & 7) == 0 && ((uintptr_t)ignored & 7) == 0 && ((uintptr_t)path_lut & 7) == 0,
                  "%s: hist, ignored and path_lut must be 8-byte aligned", who);
  CalArgs a;
  if (const int rc = dec_pack_tree(who, nlevels, C, tree, a.node, a.C)) return rc;
  if (const int rc = dec_level_pointers(who, nlevels, z, a.z)) return rc;
  a.nodes = 0;
  for (int L = 0; L < HRSEG_DECODE_MAX_LEVELS; ++L) {
    a.row0[L] = a.nodes;
    a.nodes += a.C[L];
    a.inv_temp[L] = 1.f;
    if (L < nlevels) {
      const float it = inv_temp[L];
      HRSEG_CHECK_ARG(it > 0.f && it <= 3.402823466e+38f, "%s: inv_temp[%d]=%g is not a finite positive number", who, L, (double)it);
      a.inv_temp[L] = it;
    }
  }
  // every channel's group: level 0 is one group without a parent, a child level's groups are its parents' child lists; a
  // slot past the level is a group of its own (the scans restart there)
  for (int L = 0; L < HRSEG_DECODE_MAX_LEVELS; ++L)
    for (int c = 0; c < CAL_CH; ++c) a.up[L * CAL_CH + c] = (unsigned)c | (1u << 8);
  for (int c = 0; c < a.C[0]; ++c) a.up[c] = 0u | ((unsigned)a.C[0] << 8);
  for (int L = 0; L + 1 < nlevels; ++L) {
    int owner[CAL_CH];
    for (int c = 0; c < CAL_CH; ++c) owner[c] = -1;
    for (int p = 0; p < a.C[L]; ++p) {
      const unsigned e = a.node[L * CAL_CH + p];
      const int first = (int)(e & 0xffu), kids = (int)((e >> 8) & 0xffu);
      for (int c = first; c < first + kids; ++c) {
        HRSEG_CHECK_ARG(owner[c] < 0, "%s: channel %d of level %d is in the child groups of channels %d and %d", who, c, L + 1,
                        owner[c], p);
        owner[c] = p;
        a.up[(L + 1) * CAL_CH + c] = (unsigned)first | ((unsigned)kids << 8) | ((unsigned)p << 16);
      }
    }
    for (int c = 0; c < a.C[L + 1]; ++c)
      HRSEG_CHECK_ARG(owner[c] >= 0, "%s: channel %d of level %d is in no child group", who, c, L + 1);
  }
  a.nlevels = nlevels;
  a.root_softmax = tree->root_softmax ? 1 : 0;
  a.n_bins = n_bins;
  a.per_image = per_image ? 1 : 0;
  const size_t lds = ((size_t)(a.nodes + nlevels) * (n_bins + 1) * CAL_WORDS + 1) * sizeof(u64);
  const dim3 grid((unsigned)dec_blocks_per_sample(B), (unsigned)B);
  hipLaunchKernelGGL(score_calibration_kernel, grid, dim3(CAL_TPB), lds, (hipStream_t)stream, a, gt, (const long long*)gdesc,
                     (const u64*)path_lut, (u64*)hist, (u64*)ignored, S);
  HRSEG_LAUNCH_CHECK("score_calibration");
  hrseg_count(CNT_SCORE_CALIBRATION);
  return 0;
}
