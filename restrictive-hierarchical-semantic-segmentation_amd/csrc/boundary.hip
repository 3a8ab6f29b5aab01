// Device boundary scoring: exact surface distances between predicted and ground-truth label maps, per image and tree node.
// The semantics are stated in include/hrseg.h (hrseg_score_boundaries); everything is integer arithmetic and every record
// field is a sum, a maximum or an order statistic of integers: the same bytes whatever order the blocks and atomics run in.
//
// No block waits for another one; kernel boundaries do the ordering.  HRSEG_SCORE_BOUNDARIES_LAUNCHES = 11 launches
// (family "score_boundaries"):
//   1. bd_clear_kernel zeroes the records, the selection state and the bitmaps of the workspace (the distance maps need no
//      clearing: they are read only where a bitmap has a bit).  Its block 0 also lays the images out: an exclusive scan of the
//      per-image bitmap / distance-map sizes into the table at the head of the workspace; an image whose descriptors are
//      not acceptable, or that would not fit the sizes the host computed, is flagged and skipped by every later launch.
//   2. bd_mark_kernel, grid (blocks, B): a wave takes 64 consecutive pixels of a row.  A lane turns its pixel of both maps
//      into paths (the table in LDS, its entries passed through LM_PATH_ENTRY of labelmap_common.h; the prediction's path is
//      dropped where the ground truth is unlabelled), gets the west / east neighbours' paths by shuffle and the north /
//      south ones by load, and per level and map ballots the lanes that
//      are border pixels of the same node: the two halves of the ballot ARE the two bitmap words, stored by lanes 0 and 32
//      where they are not zero.  Border pixels are counted per block in LDS, then one 64-bit atomic per non-zero cell.
//   3. bd_search_kernel, grid (blocks, 2 N, B): a block belongs to one (node, direction); it leaves at once when either set is
//      empty.  A lane reads one bitmap word of the querying set and takes its pixels one at a time.  It first tries the 7
//      rows around the pixel alone (bd_local: at most 14 words), which decides every d2 <= 16 exactly -- the outline of a
//      good prediction.  The wave ballots the queries left open and takes them one after the other, all 64 lanes on one
//      query: lane l takes the row at vertical offset d0 + l / 2 above (even l) or below (odd l), scans only the words
//      within the horizontal reach the best distance so far leaves, and the wave takes the minimum; d0 advances by 32 until
//      d0^2 >= best.  A first round with a fixed reach of 32 columns gives a middling match its bound before any long row
//      is read: no lane ever walks a long search while the others idle.  d2 goes to the int32 map of (level, direction);
//      sum_q16, max_d2 and within are kept in registers, folded over the wave, and leave as three 64-bit atomics per wave.
//   4.-11. four radix passes (8 bits each, most significant first) for the nearest-rank percentile, the method of
//      hrseg_ohem_select on integer keys: bd_hist_kernel (grid as 3.) walks the bits of the querying bitmap, reads d2 and
//      counts the digit of the keys that match the prefix chosen so far, per block in LDS, then one 32-bit atomic per
//      non-zero bin; bd_pick_kernel (one block per (image, node, direction)) scans the 256 bins, fixes the digit that
//      holds the k-th key, re-bases k, zeroes the bins for the next pass, and behind the last pass writes pk_d2.
// A node absent from either map is never searched or selected: its fields other than n keep the zeros of launch 1.
#include <limits.h>

#include "labelmap_common.h"

#define BD_TPB 256
#define BD_WAVES (BD_TPB / HRSEG_WAVE)
#define BD_MAX_LEVELS HRSEG_SCORE_MAX_LEVELS
#define BD_MAX_NODES 64
#define BD_SEG_WORDS HRSEG_BOUNDARY_SEGMENT_WORDS      // 256 bins, k, prefix, two spare: the selection state of one (image, node, direction)
#define BD_SEG_K 256
#define BD_SEG_PREFIX 257
#define BD_FIELDS 5
#define BD_PROBE 32                                    // horizontal reach of the wave's first round
#define BD_LOCAL 3                                     // rows above and below that a lane tries alone: decides d2 <= 16
#define BD_MAX_SIDE HRSEG_BOUNDARY_MAX_SIDE
#define BD_NO_IMAGE (~0ull)
#define BD_FAR (1 << 20)                               // "no bit found in this row": above every dx
static_assert(BD_SEG_WORDS == 260 && BD_TPB == 256, "one thread per radix bin; hrseg.h states the workspace formula");
static_assert(BD_MAX_SIDE == 32768, "d2 <= 2 * 32767^2 < 2^31");

struct BdArgs {
  int C[BD_MAX_LEVELS];
  int base[BD_MAX_LEVELS];                             // breadth-first index of the first node of level L
  int nlevels, N;
};

// the workspace, cut up by the host: table [B][2] u64 (word offsets of an image's bitmaps / distance maps), selection state,
// bitmaps (all images), distance maps (all images)
struct BdWs {
  u64* tab;
  u32* seg;
  u32* bm;
  int* d2;
  u64 bm_words, d2_words;
};

// words of one image's bitmaps [2 N][H][ceil(W / 32)] and distance maps [2 nlevels][H * W]
__host__ __device__ static inline void bd_image_words(long long H, long long W, int N, int nlevels, u64* bm, u64* d2) {
  *bm = (u64)(2 * N) * (u64)H * (u64)((W + 31) / 32);
  *d2 = (u64)(2 * nlevels) * (u64)H * (u64)W;
}

__host__ __device__ static inline bool bd_size_ok(long long off, long long H, long long W) {
  return off >= 0 && H >= 1 && W >= 1 && H <= BD_MAX_SIDE && W <= BD_MAX_SIDE;        // (so H * W <= 2^30)
}

struct BdImage {
  long long poff, goff;
  int H, W, wpr;
  u64 bm, d2;
  bool ok;
};

__device__ __forceinline__ bool bd_desc_ok(const long long* __restrict__ pdesc, const long long* __restrict__ gdesc, int b) {
  return bd_size_ok(pdesc[4 * b], pdesc[4 * b + 1], pdesc[4 * b + 2]) && gdesc[4 * b] >= 0 && gdesc[4 * b + 1] == pdesc[4 * b + 1] &&
         gdesc[4 * b + 2] == pdesc[4 * b + 2];
}

__device__ __forceinline__ BdImage bd_image(const BdWs& ws, const long long* __restrict__ pdesc, const long long* __restrict__ gdesc, int b) {
  BdImage im;
  im.bm = ws.tab[2 * b];
  im.d2 = ws.tab[2 * b + 1];
  im.ok = im.bm != BD_NO_IMAGE && bd_desc_ok(pdesc, gdesc, b);
  im.poff = pdesc[4 * b];
  im.goff = gdesc[4 * b];
  im.H = (int)pdesc[4 * b + 1];
  im.W = (int)pdesc[4 * b + 2];
  im.wpr = (im.W + 31) / 32;
  return im;
}

// floor(sqrt(d2 << 32)): the distance in 16.16 fixed point.  The floating-point root is a first guess only; the two loops
// make it exact with integer multiplies (s < 2^31.5, so s * s and (s + 1)^2 fit 64 bits).
__device__ __forceinline__ u64 bd_isqrt_q16(int d2) {
  const u64 v = (u64)(u32)d2 << 32;
  u64 s = (u64)sqrt((double)v);
  while (s * s > v) --s;
  while ((s + 1) * (s + 1) <= v) ++s;
  return s;
}

// ------------------------------------------------------------------------------------------------ 1. clear and lay out
__global__ __launch_bounds__(BD_TPB) void bd_clear_kernel(BdArgs a, BdWs ws, const long long* __restrict__ pdesc,
                                                          const long long* __restrict__ gdesc, int B, u64* __restrict__ records) {
  __shared__ u64 sbm[BD_TPB], sd2[BD_TPB];
  const u64 t0 = (u64)blockIdx.x * BD_TPB + threadIdx.x, stride = (u64)gridDim.x * BD_TPB;
  u64* z = reinterpret_cast<u64*>(ws.seg);                                 // selection state and bitmaps are one span
  const u64 nz = ((u64)B * a.N * 2 * BD_SEG_WORDS + ws.bm_words) / 2, nr = (u64)B * a.N * 2 * BD_FIELDS;
  for (u64 i = t0; i < nz; i += stride) z[i] = 0;
  for (u64 i = t0; i < nr; i += stride) records[i] = 0;
  if (blockIdx.x != 0) return;
  // exclusive scan of the images' sizes: a thread owns `per` consecutive images
  const int tid = threadIdx.x, per = (B + BD_TPB - 1) / BD_TPB, b0 = min(B, tid * per), b1 = min(B, b0 + per);
  u64 mb = 0, md = 0;
  for (int b = b0; b < b1; ++b) {
    if (!bd_desc_ok(pdesc, gdesc, b)) continue;
    u64 wb, wd;
    bd_image_words(pdesc[4 * b + 1], pdesc[4 * b + 2], a.N, a.nlevels, &wb, &wd);
    mb += wb;
    md += wd;
  }
  sbm[tid] = mb;
  sd2[tid] = md;
  __syncthreads();
  u64 ob = 0, od = 0;
  for (int t = 0; t < tid; ++t) {
    ob += sbm[t];
    od += sd2[t];
  }
  for (int b = b0; b < b1; ++b) {
    u64 wb = 0, wd = 0;
    bool ok = bd_desc_ok(pdesc, gdesc, b);
    if (ok) {
      bd_image_words(pdesc[4 * b + 1], pdesc[4 * b + 2], a.N, a.nlevels, &wb, &wd);
      ok = ob + wb <= ws.bm_words && od + wd <= ws.d2_words;                 // (device and host descriptors disagree: skip)
    }
    ws.tab[2 * b] = ok ? ob : BD_NO_IMAGE;
    ws.tab[2 * b + 1] = od;
    if (ok) {
      ob += wb;
      od += wd;
    }
  }
}

// ------------------------------------------------------------------------------------------------ 2. border bitmaps
// paths of pixel (yy, xx) in the prediction and the ground truth; outside the image, and where the ground truth is no
// leaf's value, both are 0: the pixel belongs to no node in either map
__device__ __forceinline__ void bd_paths(const u64* lut, const u8* __restrict__ ps, const u8* __restrict__ gs, int H, int W, int yy, int xx,
                                         u64* pe, u64* ge) {
  *pe = *ge = 0;
  if (yy < 0 || yy >= H || xx < 0 || xx >= W) return;
  const long long i = (long long)yy * W + xx;
  const u64 g = lut[gs[i]];
  if (g == 0) return;
  *ge = g;
  *pe = lut[ps[i]];
}

__global__ __launch_bounds__(BD_TPB) void bd_mark_kernel(BdArgs a, BdWs ws, const u8* __restrict__ pred, const long long* __restrict__ pdesc,
                                                         const u8* __restrict__ gt, const long long* __restrict__ gdesc,
                                                         const u64* __restrict__ path_lut, u64* __restrict__ records) {
  __shared__ u64 lut[256];
  __shared__ u32 cnt[2 * BD_MAX_NODES];
  const int b = blockIdx.y, tid = threadIdx.x, wave = tid / HRSEG_WAVE, lane = tid & (HRSEG_WAVE - 1);
  const BdImage im = bd_image(ws, pdesc, gdesc, b);
  if (!im.ok) return;
  const int H = im.H, W = im.W, cpr = (W + 63) / 64;
  const long long nchunks = (long long)H * cpr;
  if ((long long)blockIdx.x * BD_WAVES >= nchunks) return;
  {
    u64 e = path_lut[tid];                                                    // BD_TPB == 256: one table entry per thread
    LM_PATH_ENTRY(e, a)
    lut[tid] = e;
  }
  if (tid < 2 * BD_MAX_NODES) cnt[tid] = 0;
  __syncthreads();
  const u8* __restrict__ ps = pred + im.poff;
  const u8* __restrict__ gs = gt + im.goff;
  u32* __restrict__ bm = ws.bm + im.bm;
  for (long long c = (long long)blockIdx.x * BD_WAVES + wave; c < nchunks; c += (long long)gridDim.x * BD_WAVES) {
    const int y = (int)(c / cpr), x0 = (int)(c % cpr) * 64, x = x0 + lane;
    const bool in = x < W;
    u64 pc, gc, pn, gn, psn, gsn;
    bd_paths(lut, ps, gs, H, W, y, in ? x : -1, &pc, &gc);
    bd_paths(lut, ps, gs, H, W, y - 1, in ? x : -1, &pn, &gn);
    bd_paths(lut, ps, gs, H, W, y + 1, in ? x : -1, &psn, &gsn);
    u64 pw = __shfl_up(pc, 1, 64), gw = __shfl_up(gc, 1, 64), pe = __shfl_down(pc, 1, 64), ge = __shfl_down(gc, 1, 64);
    if (lane == 0) bd_paths(lut, ps, gs, H, W, y, x - 1, &pw, &gw);
    if (lane == HRSEG_WAVE - 1) bd_paths(lut, ps, gs, H, W, y, x + 1, &pe, &ge);
    for (int L = 0; L < a.nlevels; ++L) {
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int sh = 8 * L;
        const u32 me = (u32)(((m ? gc : pc) >> sh) & 0xffu);
        const bool border = in && me != 0 &&
                            ((u32)(((m ? gn : pn) >> sh) & 0xffu) != me || (u32)(((m ? gsn : psn) >> sh) & 0xffu) != me ||
                             (u32)(((m ? gw : pw) >> sh) & 0xffu) != me || (u32)(((m ? ge : pe) >> sh) & 0xffu) != me);
        u64 todo = __ballot(border);
        while (todo) {
          const int leader = __ffsll((long long)todo) - 1;
          const u32 cl = (u32)__builtin_amdgcn_readlane((int)me, leader);
          const u64 same = __ballot(border && me == cl);
          const int s = (a.base[L] + (int)cl - 1) * 2 + m;
          if ((lane & 31) == 0) {
            const u32 w = (u32)(same >> lane);                                // lane 0: columns x0 .. x0 + 31, lane 32: the next 32
            if (w) bm[((u64)s * H + y) * im.wpr + (x0 >> 5) + (lane >> 5)] = w;  // (a non-zero word lies inside the row)
          }
          if (lane == 0) atomicAdd(&cnt[s], (u32)__popcll(same));
          todo &= ~same;
        }
      }
    }
  }
  __syncthreads();
  if (tid < 2 * a.N && cnt[tid]) atomicAdd(&records[((u64)b * a.N * 2 + tid) * BD_FIELDS], (u64)cnt[tid]);
}

// ------------------------------------------------------------------------------------------------ 3. nearest distances
// smallest |dx| to a set bit of row `row` among the words that cover columns x - r .. x + r (BD_FAR: none).  Scanning a
// word more than the reach asks for is harmless: every bit found is a real pixel of the set.
// |dx| from column x to the nearest set bit of bitmap word number w of a row, whose bits are v (BD_FAR: v is 0)
__device__ __forceinline__ int bd_word_dx(u32 v, int w, int x) {
  if (v == 0) return BD_FAR;
  const int xw = x >> 5, xbit = x & 31;
  if (w < xw) return x - (w * 32 + 31 - __clz((int)v));
  if (w > xw) return w * 32 + (__ffs((int)v) - 1) - x;
  const u32 upto = 0xffffffffu >> (31 - xbit), below = v & upto, above = v & ~upto;
  int dx = BD_FAR;
  if (below) dx = xbit - (31 - __clz((int)below));
  if (above) dx = min(dx, (__ffs((int)above) - 1) - xbit);
  return dx;
}

__device__ __forceinline__ int bd_row(const u32* __restrict__ row, int W, int x, int r) {
  const int lo = max(0, x - r) >> 5, hi = min(W - 1, x + r) >> 5;
  int best = BD_FAR;
  for (int w = lo; w <= hi; ++w) best = min(best, bd_word_dx(row[w], w, x));
  return best;
}

// one query, one lane: the rows within BD_LOCAL of y, each over the words that cover x - (BD_LOCAL + 1) .. x + (BD_LOCAL + 1).
// The least candidate b is returned only when b <= (BD_LOCAL + 1)^2, and then it is exact: a pixel further than BD_LOCAL
// rows away is at least that far, and a nearer pixel within those rows has |dx| <= BD_LOCAL, inside the words scanned.
// -1: not decided here (the usual answer of a good prediction is decided here: its outline is a pixel or two off).
__device__ __forceinline__ int bd_local(const u32* __restrict__ T, int H, int W, int wpr, int y, int x) {
  // the reach of BD_LOCAL + 1 columns touches one or two words; all 14 loads are issued before the first is used
  const int a = max(0, x - (BD_LOCAL + 1)) >> 5, b = min(W - 1, x + (BD_LOCAL + 1)) >> 5;
  u32 va[2 * BD_LOCAL + 1], vb[2 * BD_LOCAL + 1];
#pragma unroll
  for (int i = 0; i <= 2 * BD_LOCAL; ++i) {
    const int yy = y + i - BD_LOCAL;
    const bool ok = yy >= 0 && yy < H;
    const u32* __restrict__ row = T + (size_t)(ok ? yy : y) * wpr;          // (a row outside the image: row y read, not used)
    const u32 la = row[a], lb = row[b];
    va[i] = ok ? la : 0u;
    vb[i] = ok ? lb : 0u;
  }
  int best = INT_MAX;
#pragma unroll
  for (int i = 0; i <= 2 * BD_LOCAL; ++i) {
    const int dy = i - BD_LOCAL, dx = min(bd_word_dx(va[i], a, x), bd_word_dx(vb[i], b, x));
    if (dx < BD_FAR) best = min(best, dy * dy + dx * dx);
  }
  return best <= (BD_LOCAL + 1) * (BD_LOCAL + 1) ? best : -1;
}

// one query, the whole wave: squared distance from (y, x) to the nearest pixel of the set T (INT_MAX: T is empty)
__device__ __forceinline__ int bd_nearest(const u32* __restrict__ T, int H, int W, int wpr, int y, int x, int lane) {
  const int dl0 = lane >> 1;
  int best;
  {
    const int yy = (lane & 1) ? y + dl0 : y - dl0;
    int cand = INT_MAX;
    if (yy >= 0 && yy < H) {
      // a reach of 32 columns touches at most three words: three loads in flight, not a loop of dependent ones
      const u32* __restrict__ row = T + (size_t)yy * wpr;
      const int a = max(0, x - BD_PROBE) >> 5, m = x >> 5, b = min(W - 1, x + BD_PROBE) >> 5;
      const u32 va = row[a], vm = row[m], vb = row[b];
      const int dx = min(bd_word_dx(vm, m, x), min(bd_word_dx(va, a, x), bd_word_dx(vb, b, x)));
      if (dx < BD_FAR) cand = dl0 * dl0 + dx * dx;
    }
    best = lm_wave_min(cand);
  }
  // bounded: d0 grows by 32 per round and the loop ends once the rows at offset d0 lie outside the image on both sides
  for (int d0 = 0; d0 <= y || d0 <= H - 1 - y; d0 += 32) {
    if (best != INT_MAX && (long long)d0 * d0 >= best) break;
    const int dl = d0 + dl0, yy = (lane & 1) ? y + dl : y - dl;
    int cand = INT_MAX;
    if (yy >= 0 && yy < H && (best == INT_MAX || dl * dl < best)) {
      // reach: any r >= sqrt(best - dl^2) is exact; the float root errs by far less than the 1 added
      const int r = best == INT_MAX ? W : (int)sqrtf((float)(best - dl * dl)) + 1;
      const int dx = bd_row(T + (size_t)yy * wpr, W, x, r);
      if (dx < BD_FAR) cand = dl * dl + dx * dx;
    }
    best = min(best, lm_wave_min(cand));
  }
  return best;
}

struct BdSeg {
  int node, dir, L;
  bool active;
};

// the (node, direction) of a block and whether both of its sets have pixels
__device__ __forceinline__ BdSeg bd_segment(const BdArgs& a, const u64* __restrict__ records, int b, int s) {
  BdSeg g;
  g.node = s >> 1;
  g.dir = s & 1;
  g.L = 0;
  for (int L = 1; L < a.nlevels; ++L)
    if (g.node >= a.base[L]) g.L = L;
  const u64* rec = records + ((u64)b * a.N + g.node) * 2 * BD_FIELDS;
  g.active = rec[0] != 0 && rec[BD_FIELDS] != 0;
  return g;
}

__global__ __launch_bounds__(BD_TPB) void bd_search_kernel(BdArgs a, BdWs ws, const long long* __restrict__ pdesc,
                                                           const long long* __restrict__ gdesc, long long tau2, u64* __restrict__ records) {
  const int s = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, wave = tid / HRSEG_WAVE, lane = tid & (HRSEG_WAVE - 1);
  const BdImage im = bd_image(ws, pdesc, gdesc, b);
  if (!im.ok) return;
  const BdSeg g = bd_segment(a, records, b, s);
  if (!g.active) return;
  const int H = im.H, W = im.W, wpr = im.wpr, nwords = H * wpr;                 // H * wpr <= 32768 * 1024
  const u32* __restrict__ Q = ws.bm + im.bm + (u64)s * nwords;
  const u32* __restrict__ T = ws.bm + im.bm + (u64)(s ^ 1) * nwords;
  int* __restrict__ D = ws.d2 + im.d2 + (u64)(g.L * 2 + g.dir) * ((u64)H * W);
  u64 sum = 0, within = 0;                                                    // per lane; folded over the wave at the end
  int far = -1;
  // words are dealt out in groups of 16 (one 64-byte line), consecutive groups to consecutive waves, four groups per wave
  // and round: the far queries of one stretch of outline, which cost the whole wave each, spread over many waves
  const long long nwaves = (long long)gridDim.x * BD_WAVES, me = (long long)blockIdx.x * BD_WAVES + wave, ngroups = (nwords + 15) / 16;
  for (long long g0 = 0; g0 < ngroups; g0 += 4 * nwaves) {
    const long long wi = (g0 + (lane >> 4) * nwaves + me) * 16 + (lane & 15);
    u32 w = wi < nwords ? Q[wi] : 0u;
    const int y = (int)(wi / wpr), xb = (int)(wi % wpr) * 32;
    while (__ballot(w != 0)) {
      // every lane takes the next pixel of its own word and tries the few rows around it alone ...
      const bool has = w != 0;
      int x = 0, d2 = -1;
      if (has) {
        x = xb + __ffs((int)w) - 1;
        w &= w - 1;
        d2 = bd_local(T, H, W, wpr, y, x);
      }
      // ... and the wave takes the queries that left open one after the other, all 64 lanes on each
      u64 open = __ballot(has && d2 < 0);
      while (open) {
        const int src = __ffsll((long long)open) - 1;
        open &= open - 1;
        const int r = bd_nearest(T, H, W, wpr, __builtin_amdgcn_readlane(y, src), __builtin_amdgcn_readlane(x, src), lane);
        if (lane == src) d2 = r;
      }
      if (has && d2 >= 0 && d2 != INT_MAX) {                                  // (INT_MAX cannot happen: the other set has pixels)
        D[(long long)y * W + x] = d2;
        sum += bd_isqrt_q16(d2);
        within += (long long)d2 <= tau2 ? 1 : 0;
        far = max(far, d2);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    within += __shfl_xor(within, o, 64);
    far = max(far, __shfl_xor(far, o, 64));
  }
  if (lane == 0 && far >= 0) {
    u64* rec = records + ((u64)b * a.N * 2 + s) * BD_FIELDS;
    atomicAdd(&rec[1], sum);
    atomicMax(&rec[2], (u64)far);
    if (within) atomicAdd(&rec[3], within);
  }
}

// ------------------------------------------------------------------------------------------------ 4. nearest-rank select
// (the digits go through lm_wave_add: real outlines have a few distances many times)
__global__ __launch_bounds__(BD_TPB) void bd_hist_kernel(BdArgs a, BdWs ws, const long long* __restrict__ pdesc,
                                                         const long long* __restrict__ gdesc, int shift, const u64* __restrict__ records) {
  __shared__ u32 hist[256];
  const int s = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, wave = tid / HRSEG_WAVE, lane = tid & (HRSEG_WAVE - 1);
  const BdImage im = bd_image(ws, pdesc, gdesc, b);
  if (!im.ok) return;
  const BdSeg g = bd_segment(a, records, b, s);
  if (!g.active) return;
  const int H = im.H, W = im.W, wpr = im.wpr, nwords = H * wpr;
  if ((long long)blockIdx.x * BD_TPB >= nwords) return;
  const u32* __restrict__ Q = ws.bm + im.bm + (u64)s * nwords;
  const int* __restrict__ D = ws.d2 + im.d2 + (u64)(g.L * 2 + g.dir) * ((u64)H * W);
  u32* seg = ws.seg + ((u64)b * a.N * 2 + s) * BD_SEG_WORDS;
  const u32 prefix = shift == 24 ? 0u : seg[BD_SEG_PREFIX];
  hist[tid] = 0;
  __syncthreads();
  for (long long base = ((long long)blockIdx.x * BD_WAVES + wave) * HRSEG_WAVE; base < nwords; base += (long long)gridDim.x * BD_TPB) {
    const long long wi = base + lane;
    u32 w = wi < nwords ? Q[wi] : 0u;
    const int y = (int)(wi / wpr), xb = (int)(wi % wpr) * 32;
    while (__ballot(w != 0)) {
      const bool has = w != 0;
      u32 v = 0;
      if (has) {
        v = (u32)D[(long long)y * W + xb + __ffs((int)w) - 1];
        w &= w - 1;
      }
      const bool match = has && (shift == 24 || (v >> (shift + 8)) == (prefix >> (shift + 8)));
      lm_wave_add(hist, (v >> shift) & 0xffu, 1u, match, lane);
    }
  }
  __syncthreads();
  if (hist[tid]) atomicAdd(&seg[tid], hist[tid]);
}

__global__ __launch_bounds__(BD_TPB) void bd_pick_kernel(BdArgs a, BdWs ws, int shift, int percentile, u64* __restrict__ records) {
  __shared__ u32 wave_total[BD_WAVES];
  const int s = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, wave = tid / HRSEG_WAVE, lane = tid & (HRSEG_WAVE - 1);
  if (ws.tab[2 * b] == BD_NO_IMAGE) return;
  const BdSeg g = bd_segment(a, records, b, s);
  if (!g.active) return;
  u64* rec = records + ((u64)b * a.N * 2 + s) * BD_FIELDS;
  u32* seg = ws.seg + ((u64)b * a.N * 2 + s) * BD_SEG_WORDS;
  // k-th smallest, k = ceil(percentile * n / 100) in 1..n; later passes: what is left of k inside the chosen prefix
  const u32 k = shift == 24 ? (u32)(((u64)percentile * rec[0] + 99) / 100) : seg[BD_SEG_K];
  const u32 prefix = shift == 24 ? 0u : seg[BD_SEG_PREFIX];
  const u32 h = seg[tid];
  u32 incl = h;
#pragma unroll
  for (int o = 1; o < HRSEG_WAVE; o <<= 1) {
    const u32 t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == HRSEG_WAVE - 1) wave_total[wave] = incl;
  __syncthreads();                                                            // (also: everybody has read k and prefix)
  for (int w = 0; w < wave; ++w) incl += wave_total[w];
  seg[tid] = 0;
  if (incl >= k && incl - h < k) {                                            // exactly one bin holds the k-th key
    const u32 p = prefix | ((u32)tid << shift);
    seg[BD_SEG_K] = k - (incl - h);
    seg[BD_SEG_PREFIX] = p;
    if (shift == 0) rec[4] = p;
  }
}

// ------------------------------------------------------------------------------------------------------------ C ABI
static int bd_levels(const char* who, int nlevels, const int* C, BdArgs* a) {
  HRSEG_CHECK_ARG(nlevels >= 1 && nlevels <= BD_MAX_LEVELS, "%s: nlevels=%d not in 1..%d", who, nlevels, BD_MAX_LEVELS);
  a->nlevels = nlevels;
  a->N = 0;
  for (int L = 0; L < BD_MAX_LEVELS; ++L) a->C[L] = a->base[L] = 0;
  for (int L = 0; L < nlevels; ++L) {
    HRSEG_CHECK_ARG(C[L] >= 1 && C[L] <= HRSEG_SCORE_MAX_CHANNELS, "%s: C[%d]=%d not in 1..%d", who, L, C[L], HRSEG_SCORE_MAX_CHANNELS);
    a->C[L] = C[L];
    a->base[L] = a->N;
    a->N += C[L];
  }
  HRSEG_CHECK_ARG(a->N <= BD_MAX_NODES, "%s: %d nodes over all levels, at most %d", who, a->N, BD_MAX_NODES);
  return 0;
}

// rows [0, B) of the host table: every image acceptable (lm_host_image, then this unit's side limit) -> words of all bitmaps / distance maps, words and chunks of the largest
static int bd_scan(const char* who, const long* desc_host, int B, const BdArgs& a, u64* bm_words, u64* d2_words, long long* max_words,
                   long long* max_chunks) {
  *bm_words = *d2_words = 0;
  *max_words = *max_chunks = 0;
  for (int b = 0; b < B; ++b) {
    long long off, H, W;
    if (int rc = lm_host_image(who, "", desc_host, b, &off, &H, &W)) return rc;
    HRSEG_CHECK_ARG(H <= BD_MAX_SIDE && W <= BD_MAX_SIDE, "%s: image %d: %lld x %lld, a side above %d", who, b, H, W, BD_MAX_SIDE);
    u64 wb, wd;
    bd_image_words(H, W, a.N, a.nlevels, &wb, &wd);
    *bm_words += wb;
    *d2_words += wd;
    const long long words = H * ((W + 31) / 32), chunks = H * ((W + 63) / 64);
    *max_words = words > *max_words ? words : *max_words;
    *max_chunks = chunks > *max_chunks ? chunks : *max_chunks;
  }
  *bm_words += *bm_words & 1;                                                 // the clear writes 8 bytes at a time
  return 0;
}

extern "C" size_t hrseg_boundary_workspace_bytes(const long* desc_host, int B, int nlevels, const int* C) {
  BdArgs a;
  u64 bm_words, d2_words;
  long long max_words, max_chunks;
  if (!desc_host || !C || B < 1 || B > 65535) {
    hrseg_set_error("hrseg_boundary_workspace_bytes: bad arguments");
    return 0;
  }
  if (bd_levels("hrseg_boundary_workspace_bytes", nlevels, C, &a)) return 0;
  if (bd_scan("hrseg_boundary_workspace_bytes", desc_host, B, a, &bm_words, &d2_words, &max_words, &max_chunks)) return 0;
  return (size_t)B * 16 + ((size_t)B * a.N * 2 * BD_SEG_WORDS + bm_words + d2_words) * 4;
}

extern "C" int hrseg_score_boundaries(const unsigned char* pred, const long* pdesc, const unsigned char* gt, const long* gdesc,
                                      const long* desc_host, const unsigned long long* path_lut, int nlevels, const int* C, long tau2,
                                      int percentile, long long* records, void* workspace, int B, hrseg_stream_t stream) {
  const char* who = "hrseg_score_boundaries";
  HRSEG_CHECK_ARG(pred && pdesc && gt && gdesc && desc_host && path_lut && C && records && workspace, "%s: null pointer", who);
  HRSEG_CHECK_ARG(B >= 1 && B <= 65535, "%s: B=%d not in 1..65535", who, B);
  HRSEG_CHECK_ARG(((uintptr_t)records & 7) == 0 && ((uintptr_t)workspace & 7) == 0 && ((uintptr_t)path_lut & 7) == 0,
                  "%s: records, workspace and path_lut must be 8-byte aligned", who);
  HRSEG_CHECK_ARG(percentile >= 1 && percentile <= 100, "%s: percentile %d not in 1..100", who, percentile);
  HRSEG_CHECK_ARG(tau2 >= 0, "%s: tau2 %ld is negative", who, tau2);
  BdArgs a;
  if (int rc = bd_levels(who, nlevels, C, &a)) return rc;
  BdWs ws;
  long long max_words, max_chunks;
  if (int rc = bd_scan(who, desc_host, B, a, &ws.bm_words, &ws.d2_words, &max_words, &max_chunks)) return rc;
  u64 gb, gd;
  long long gw, gc;
  if (int rc = bd_scan(who, desc_host + 4 * (size_t)B, B, a, &gb, &gd, &gw, &gc)) return rc;
  if (int rc = lm_host_same_sizes(who, desc_host, B)) return rc;
  ws.tab = (u64*)workspace;
  ws.seg = (u32*)((char*)workspace + (size_t)B * 16);
  ws.bm = ws.seg + (size_t)B * a.N * 2 * BD_SEG_WORDS;
  ws.d2 = (int*)(ws.bm + ws.bm_words);
  const hipStream_t st = (hipStream_t)stream;
  const long long* pd = (const long long*)pdesc;
  const long long* gdv = (const long long*)gdesc;
  u64* rec = (u64*)records;

  const u64 clear_words = ((u64)B * a.N * 2 * BD_SEG_WORDS + ws.bm_words) / 2;
  const unsigned clear_blocks = (unsigned)(clear_words / (BD_TPB * 8) > 2047 ? 2048 : clear_words / (BD_TPB * 8) + 1);
  hipLaunchKernelGGL(bd_clear_kernel, dim3(clear_blocks), dim3(BD_TPB), 0, st, a, ws, pd, gdv, B, rec);
  HRSEG_LAUNCH_CHECK("score_boundaries (clear)");
  long long mark_blocks = (max_chunks + BD_WAVES * 8 - 1) / (BD_WAVES * 8);     // a wave takes about 8 chunks
  mark_blocks = mark_blocks > 4096 ? 4096 : mark_blocks;
  hipLaunchKernelGGL(bd_mark_kernel, dim3((unsigned)mark_blocks, (unsigned)B), dim3(BD_TPB), 0, st, a, ws, pred, pd, gt, gdv,
                     (const u64*)path_lut, rec);
  HRSEG_LAUNCH_CHECK("score_boundaries (mark)");
  long long scan_blocks = (max_words + BD_TPB - 1) / BD_TPB;
  scan_blocks = scan_blocks > 128 ? 128 : scan_blocks;
  const dim3 scan_grid((unsigned)scan_blocks, (unsigned)(2 * a.N), (unsigned)B);
  hipLaunchKernelGGL(bd_search_kernel, scan_grid, dim3(BD_TPB), 0, st, a, ws, pd, gdv, (long long)tau2, rec);
  HRSEG_LAUNCH_CHECK("score_boundaries (search)");
  for (int shift = 24; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(bd_hist_kernel, scan_grid, dim3(BD_TPB), 0, st, a, ws, pd, gdv, shift, (const u64*)rec);
    HRSEG_LAUNCH_CHECK("score_boundaries (histogram)");
    hipLaunchKernelGGL(bd_pick_kernel, dim3((unsigned)(2 * a.N), (unsigned)B), dim3(BD_TPB), 0, st, a, ws, shift, percentile, rec);
    HRSEG_LAUNCH_CHECK("score_boundaries (pick)");
  }
  hrseg_count(CNT_SCORE_BOUNDARIES, HRSEG_SCORE_BOUNDARIES_LAUNCHES);
  return 0;
}
