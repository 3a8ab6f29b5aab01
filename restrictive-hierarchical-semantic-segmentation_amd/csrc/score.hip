// Device scoring pipeline: a batch of predicted uint8 label maps against ground-truth maps of the same (ragged) sizes ->
// per-level confusion counts in the (target, predicted) layout hrseg_metric_vectors reads, plus the two "ignored" counts.
// The semantics are stated in include/hrseg.h (hrseg_score_labels).  Everything is integer arithmetic, and the counts
// are sums of integers: the same bits whatever the block order, so there is no deterministic variant.
//
// One launch (family "score_labels"), grid (blocks, B): every sample gets the same number of blocks (its size is known
// on the device only), which stride over the sample's block-steps of SCORE_BLOCK_STEP pixels; a block past the sample's
// last step leaves at once.  The kernel reads 2 bytes per pixel; what it has to manage is contention: real maps are
// dominated by one pair (background on background).  So a block counts PAIRS OF LEAVES, not cells of the level
// matrices, and folds equal pairs three times before an LDS atomic is issued:
//   0. setup: thread v reads path_lut[v], drops an entry that is no leaf (LM_PATH_ENTRY, labelmap_common.h), and numbers
//      the remaining ones (ballot + popcount prefix): leaf ids 1..NL <= 64 per byte value, the path of every leaf id.
//   1. a lane takes SCORE_LANE_STEP = 16 consecutive pixels of both maps.  The lane steps are cut at 16-byte boundaries of
//      the PREDICTION span (one aligned 16-byte load); the ground-truth span starts at an unrelated byte, so the lane
//      loads the 5 aligned dwords around its 16 bytes and funnel-shifts them (v_alignbyte).  Lanes whose 16 pixels or whose
//      aligned windows would leave [offset, offset + H*W) of either buffer -- only the first and last of an image --
//      load single bytes instead.  Runs fold in three tiers: all 16 pixels one pair / a dword of 4 pixels one pair /
//      single pixels; a tier runs only when some lane of the wave needs it.
//   2. inside a tier every participating lane holds one key and the same count (16, 4 or 1): equal keys of a wave are
//      folded before the LDS atomic (lm_wave_add, labelmap_common.h).
//   3. LDS: a 64 x 64 histogram of leaf pairs (+ the two ignored counts), 32-bit: a block counts pixels of ONE image,
//      H*W <= 2^31.
// Flush: every non-zero pair is expanded into one cell per level of a second LDS array (the level matrices, side by side),
// whose non-zero cells go to the int64 counts with one 64-bit atomic add each.
#include "labelmap_common.h"

#define SCORE_TPB 256
#define SCORE_LANE_STEP HRSEG_SCORE_LANE_STEP       // 16: the tests take the three step sizes from the header
#define SCORE_WAVE_STEP HRSEG_SCORE_WAVE_STEP
#define SCORE_BLOCK_STEP HRSEG_SCORE_BLOCK_STEP
static_assert(SCORE_LANE_STEP == 16 && SCORE_WAVE_STEP == HRSEG_WAVE * SCORE_LANE_STEP && SCORE_BLOCK_STEP == SCORE_TPB * SCORE_LANE_STEP,
              "hrseg.h states the step sizes of this kernel");
#define SCORE_MAX_LEAVES 64
#define SCORE_PAIRS (SCORE_MAX_LEAVES * SCORE_MAX_LEAVES)
#define SCORE_IGN_GT SCORE_PAIRS                   // histogram slots behind the pairs
#define SCORE_IGN_PRED (SCORE_PAIRS + 1)
#define SCORE_MAX_CELLS (HRSEG_SCORE_MAX_CHANNELS * HRSEG_SCORE_MAX_CHANNELS + \
                         (HRSEG_SCORE_MAX_LEVELS - 1) * (HRSEG_SCORE_MAX_CHANNELS + 1) * (HRSEG_SCORE_MAX_CHANNELS + 1))
#define SCORE_BLOCKS 1024                          // blocks of a launch, over all samples

struct ScoreArgs {
  int C[HRSEG_SCORE_MAX_LEVELS];
  int off[HRSEG_SCORE_MAX_LEVELS];                 // first cell of level L in a row of counts
  int nlevels, total, per_image;
};

// 16 pixels of both maps: byte j of dword d is pixel 4 d + j; bit 4 d + j of `valid` says the pixel exists
struct ScoreTile {
  unsigned p[4], g[4], valid;
};

__device__ __forceinline__ ScoreTile score_load(const u8* __restrict__ pred, const u8* __restrict__ gt, long long i0, long long HW) {
  ScoreTile t;
  t.valid = 0;
#pragma unroll
  for (int d = 0; d < 4; ++d) t.p[d] = t.g[d] = 0;
  if (i0 >= HW || i0 + SCORE_LANE_STEP <= 0) return t;
  const uintptr_t ga = (uintptr_t)gt + (uintptr_t)i0, fa = ga & ~(uintptr_t)3;
  const bool inside = i0 >= 0 && i0 + SCORE_LANE_STEP <= HW;
  if (inside && fa >= (uintptr_t)gt && fa + 20 <= (uintptr_t)gt + (uintptr_t)HW) {
    const u32x4 pv = *reinterpret_cast<const u32x4*>(pred + i0);       // pred + i0 is 16-byte aligned
    const unsigned* __restrict__ gw = reinterpret_cast<const unsigned*>(fa);
    const unsigned w0 = gw[0], w1 = gw[1], w2 = gw[2], w3 = gw[3], w4 = gw[4];
    const unsigned sh = (unsigned)(ga & 3);
    t.p[0] = pv[0];
    t.p[1] = pv[1];
    t.p[2] = pv[2];
    t.p[3] = pv[3];
    t.g[0] = __builtin_amdgcn_alignbyte(w1, w0, sh);
    t.g[1] = __builtin_amdgcn_alignbyte(w2, w1, sh);
    t.g[2] = __builtin_amdgcn_alignbyte(w3, w2, sh);
    t.g[3] = __builtin_amdgcn_alignbyte(w4, w3, sh);
    t.valid = 0xffffu;
    return t;
  }
#pragma unroll
  for (int d = 0; d < 4; ++d) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long i = i0 + 4 * d + j;
      if (i >= 0 && i < HW) {
        t.p[d] |= (unsigned)pred[i] << (8 * j);
        t.g[d] |= (unsigned)gt[i] << (8 * j);
        t.valid |= 1u << (4 * d + j);
      }
    }
  }
  return t;
}

// histogram slot of one (ground truth, prediction) byte pair
__device__ __forceinline__ unsigned score_key(const u8* leafid, unsigned g, unsigned p) {
  const unsigned gi = leafid[g], pi = leafid[p];
  return gi == 0 ? SCORE_IGN_GT : (pi == 0 ? SCORE_IGN_PRED : (gi - 1) * SCORE_MAX_LEAVES + (pi - 1));
}

__device__ __forceinline__ void score_count(unsigned* hist, const u8* leafid, const ScoreTile& t, int lane) {
  if (__ballot(t.valid != 0) == 0) return;
  const unsigned p0 = (t.p[0] & 0xffu) * 0x01010101u, g0 = (t.g[0] & 0xffu) * 0x01010101u;
  const bool one = t.valid == 0xffffu && t.p[0] == p0 && t.p[1] == p0 && t.p[2] == p0 && t.p[3] == p0 && t.g[0] == g0 &&
                   t.g[1] == g0 && t.g[2] == g0 && t.g[3] == g0;
  lm_wave_add(hist, score_key(leafid, t.g[0] & 0xffu, t.p[0] & 0xffu), SCORE_LANE_STEP, one, lane);
  const bool rest = !one && t.valid != 0;
  if (__ballot(rest) == 0) return;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const unsigned pd = t.p[d], gd = t.g[d], vd = (t.valid >> (4 * d)) & 0xfu;
    const bool four = rest && vd == 0xfu && pd == (pd & 0xffu) * 0x01010101u && gd == (gd & 0xffu) * 0x01010101u;
    lm_wave_add(hist, score_key(leafid, gd & 0xffu, pd & 0xffu), 4, four, lane);
    const bool single = rest && !four && vd != 0;
    if (__ballot(single) == 0) continue;
    for (int j = 0; j < 4; ++j) {
      const bool has = single && ((vd >> j) & 1u);
      lm_wave_add(hist, score_key(leafid, (gd >> (8 * j)) & 0xffu, (pd >> (8 * j)) & 0xffu), 1, has, lane);
    }
  }
}

__global__ __launch_bounds__(SCORE_TPB) void score_labels_kernel(ScoreArgs a, const u8* __restrict__ pred,
                                                                 const long long* __restrict__ pdesc, const u8* __restrict__ gt,
                                                                 const long long* __restrict__ gdesc, const u64* __restrict__ path_lut,
                                                                 u64* __restrict__ counts, u64* __restrict__ ignored) {
  __shared__ unsigned hist[SCORE_PAIRS + 2];
  __shared__ unsigned cells[SCORE_MAX_CELLS];
  __shared__ u64 leafpath[SCORE_MAX_LEAVES];
  __shared__ u8 leafid[256];
  __shared__ int wave_leaves[SCORE_TPB / HRSEG_WAVE];
  const int b = blockIdx.y, tid = threadIdx.x, wave = tid / HRSEG_WAVE, lane = tid & (HRSEG_WAVE - 1);
  const long long poff = pdesc[4 * b], H = pdesc[4 * b + 1], W = pdesc[4 * b + 2];
  const long long goff = gdesc[4 * b], gH = gdesc[4 * b + 1], gW = gdesc[4 * b + 2];
  if (H < 1 || W < 1 || H != gH || W != gW || poff < 0 || goff < 0) return;
  if (H > (1ll << 31) / W) return;                                     // H*W > 2^31: the 32-bit block counts could wrap
  const long long HW = H * W;
  const u8* __restrict__ ps = pred + poff;
  const u8* __restrict__ gs = gt + goff;
  const int mis = (int)((uintptr_t)ps & (SCORE_LANE_STEP - 1));          // ps - mis is 16-byte aligned
  const long long nsteps = (HW + mis + SCORE_BLOCK_STEP - 1) / SCORE_BLOCK_STEP;
  if ((long long)blockIdx.x >= nsteps) return;

  // ---- setup: zero the counters, number the leaves
  for (int i = tid; i < SCORE_PAIRS + 2; i += SCORE_TPB) hist[i] = 0;
  for (int i = tid; i < a.total; i += SCORE_TPB) cells[i] = 0;
  u64 e = path_lut[tid];                                               // SCORE_TPB == 256: one table entry per thread
  LM_PATH_ENTRY(e, a)
  const u64 nz = __ballot(e != 0);
  if (lane == 0) wave_leaves[wave] = __popcll(nz);
  __syncthreads();
  int id = __popcll(nz & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) id += wave_leaves[w];
  const bool leaf = e != 0 && id < SCORE_MAX_LEAVES;
  leafid[tid] = leaf ? (u8)(id + 1) : (u8)0;
  if (leaf) leafpath[id] = e;
  __syncthreads();

  // ---- count leaf pairs; the next step's loads are in flight while this one is counted
  const long long stride = (long long)gridDim.x * SCORE_BLOCK_STEP;
  long long i0 = ((long long)blockIdx.x * SCORE_TPB + tid) * SCORE_LANE_STEP - mis;
  ScoreTile cur = score_load(ps, gs, i0, HW);
  for (long long s = blockIdx.x; s < nsteps; s += gridDim.x) {
    i0 += stride;
    const ScoreTile nxt = score_load(ps, gs, i0, HW);                   // past the image: an empty tile, nothing is read
    score_count(hist, leafid, cur, lane);
    cur = nxt;
  }
  __syncthreads();

  // ---- pairs -> cells of the level matrices (LDS) -> int64 counts
  for (int i = tid; i < SCORE_PAIRS; i += SCORE_TPB) {
    const unsigned n = hist[i];
    if (n == 0) continue;
    const u64 g = leafpath[i / SCORE_MAX_LEAVES], p = leafpath[i % SCORE_MAX_LEAVES];
    int gp = (int)(g & 0xffu), pp = (int)(p & 0xffu);
    atomicAdd(&cells[(gp - 1) * a.C[0] + (pp - 1)], n);
    for (int L = 1; L < a.nlevels; ++L) {
      const int gl = (int)((g >> (8 * L)) & 0xffu), pl = (int)((p >> (8 * L)) & 0xffu);
      atomicAdd(&cells[a.off[L] + gl * (a.C[L] + 1) + (gp == pp ? pl : 0)], n);
      gp = gl;
      pp = pl;
    }
  }
  __syncthreads();
  const size_t row = a.per_image ? (size_t)b : 0;
  for (int i = tid; i < a.total; i += SCORE_TPB)
    if (cells[i]) atomicAdd(&counts[row * a.total + i], (u64)cells[i]);
  if (tid < 2 && hist[SCORE_PAIRS + tid]) atomicAdd(&ignored[row * 2 + tid], (u64)hist[SCORE_PAIRS + tid]);
}

// ------------------------------------------------------------------------------------------------------------ C ABI
extern "C" int hrseg_score_labels(const unsigned char* pred, const long* pdesc, const unsigned char* gt, const long* gdesc,
                                  const unsigned long long* path_lut, int nlevels, const int* C, long long* counts,
                                  long long* ignored, int B, int per_image, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(pred && pdesc && gt && gdesc && path_lut && C && counts && ignored && B > 0 && B <= 65535,
                  "hrseg_score_labels: bad arguments");
  HRSEG_CHECK_ARG(nlevels >= 1 && nlevels <= HRSEG_SCORE_MAX_LEVELS, "hrseg_score_labels: nlevels=%d not in 1..%d", nlevels,
                  HRSEG_SCORE_MAX_LEVELS);
  HRSEG_CHECK_ARG(((uintptr_t)counts & 7) == 0 && ((uintptr_t)ignored & 7) == 0 && ((uintptr_t)path_lut & 7) == 0,
                  "hrseg_score_labels: counts, ignored and path_lut must be 8-byte aligned");
  ScoreArgs a;
  int channels = 0;
  a.total = 0;
  for (int L = 0; L < HRSEG_SCORE_MAX_LEVELS; ++L) a.C[L] = a.off[L] = 0;
  for (int L = 0; L < nlevels; ++L) {
    HRSEG_CHECK_ARG(C[L] >= 1 && C[L] <= HRSEG_SCORE_MAX_CHANNELS, "hrseg_score_labels: C[%d]=%d not in 1..%d", L, C[L],
                    HRSEG_SCORE_MAX_CHANNELS);
    const int K = C[L] + (L > 0 ? 1 : 0);
    a.C[L] = C[L];
    a.off[L] = a.total;
    a.total += K * K;
    channels += C[L];
  }
  HRSEG_CHECK_ARG(channels <= 64, "hrseg_score_labels: %d channels over all levels, at most 64", channels);
  a.nlevels = nlevels;
  a.per_image = per_image ? 1 : 0;
  int per_sample = (SCORE_BLOCKS + B - 1) / B;
  per_sample = per_sample < 1 ? 1 : per_sample;
  hipLaunchKernelGGL(score_labels_kernel, dim3((unsigned)per_sample, (unsigned)B), dim3(SCORE_TPB), 0, (hipStream_t)stream, a,
                     pred, (const long long*)pdesc, gt, (const long long*)gdesc, (const u64*)path_lut, (u64*)counts, (u64*)ignored);
  HRSEG_LAUNCH_CHECK("score_labels");
  hrseg_count(CNT_SCORE_LABELS);
  return 0;
}
