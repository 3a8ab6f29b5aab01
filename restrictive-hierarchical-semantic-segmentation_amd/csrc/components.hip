// Device post-processing: connected components of ragged uint8 label maps and the area / keep-largest filter on them.
// The semantics are stated in include/hrseg.h (hrseg_label_components, hrseg_filter_components); everything is integer
// arithmetic and every result is defined by row-major order, so two runs give the same bytes whatever the block order.
//
// Union-find over the pixels of one image, the parent array living in `roots`.  The one invariant: parent[i] <= i, at all
// times, for every pixel.  A union links the LARGER of two roots below the smaller (atomicMin), so
//   - every find is a strictly descending walk: at most i steps from pixel i;
//   - a root is the smallest index of its set, so the final root of a component is its first pixel in row-major order,
//     whatever order the atomics land in;
//   - a stale read of a parent (another XCD's L2) is an older, larger ancestor of the same set: the walk is longer, never
//     wrong, and a link is only ever made by an atomicMin, which acts on the current value.
// No block waits for another one: the only cross-block traffic inside a launch are atomicMin on parents, atomicAdd on areas
// and statistics and the 64-bit atomicMax on the per-group best word; kernel boundaries do the ordering.
//
// hrseg_label_components, 3 launches (family "label_components"), grid (tiles of the largest image, B):
//   1. cc_tile_kernel: a block labels one CC_TW x CC_TH tile in LDS (group ids from 16-byte loads of the label rows; runs of
//      8 pixels sequentially, the rest by LDS atomicMin) and writes each pixel's tile-local root as an image index; area = 0.
//   2. cc_merge_kernel: the pixels of a tile's top row and left column union with their neighbours in the tiles above /
//      left of them (global atomicMin).  A union is left out where two others of the same launch imply it, so a uniform
//      region costs one union per tile edge, not one per border pixel.
//   3. cc_flatten_kernel: every pixel walks to its root and stores it; areas: a thread folds its 8 pixels into runs, the
//      block adds the runs of its first pixel's root once, the wave adds equal roots once (CC_PEEL rounds), the rest
//      add for themselves (many distinct roots: no contention).
// hrseg_filter_components, 3 launches (family "filter_components"), grid (steps, B):
//   4. cc_clear_kernel zeroes the workspace; cc_best_kernel: per image and group the 64-bit maximum of (area << 32 | ~first pixel) over the components, folded per
//      block in LDS first.
//   5. cc_filter_kernel: 16 pixels per lane (one aligned 16-byte load of the labels where the span allows), the verdict of
//      a root is kept from pixel to pixel; statistics per block in LDS, then one 64-bit atomicAdd per non-zero cell.
#include "labelmap_common.h"

#define CC_TW HRSEG_COMPONENTS_TILE_W
#define CC_TH HRSEG_COMPONENTS_TILE_H
#define CC_TPB 256
#define CC_RUN 8                                   // consecutive pixels of a row per thread
static_assert(CC_TW == 64 && CC_TH == 32 && CC_TW * CC_TH == CC_TPB * CC_RUN && CC_TW % CC_RUN == 0,
              "a thread owns 8 consecutive pixels of a tile row");
#define CC_CHUNKS (CC_TW / 16 + 1)                 // aligned 16-byte windows a tile row can touch
#define CC_MERGE_TPB 128
static_assert(CC_TW + CC_TH <= CC_MERGE_TPB, "one thread per pixel of a tile's top row and left column");
#define CC_PEEL 4
#define CC_STEP 16                                 // pixels per lane in the filter
#define CC_BEST_STEP 4                             // pixels per thread in the maximum

struct CcImage {
  long long off;
  int H, W;
  bool ok;
};

__device__ __forceinline__ CcImage cc_image(const long long* __restrict__ desc, int b) {
  CcImage im;
  const long long H = desc[4 * b + 1], W = desc[4 * b + 2];
  im.off = desc[4 * b];
  im.ok = H >= 1 && W >= 1 && im.off >= 0 && H <= ((1ll << 31) - 1) / W;          // H*W < 2^31
  im.H = (int)H;
  im.W = (int)W;
  return im;
}

// ---- union-find.  LDS (block scope) and global (device scope) variants of the same two loops.
template <bool GLOBAL>
__device__ __forceinline__ int cc_load(const int* p) {
  if (GLOBAL) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <bool GLOBAL>
__device__ __forceinline__ int cc_find(const int* P, int i) {
  // bounded: parent[i] <= i, so the index strictly falls until it meets a root: at most i steps
  for (int p = cc_load<GLOBAL>(P + i); p != i; p = cc_load<GLOBAL>(P + i)) i = p;
  return i;
}
template <bool GLOBAL>
__device__ __forceinline__ void cc_union(int* P, int a, int b) {
  // bounded: an iteration either returns or goes on with a strictly smaller `a` (old < a: somebody else lowered that
  // parent, and the walk from old only descends), so there are at most max(a, b) iterations
  for (;;) {
    a = cc_find<GLOBAL>(P, a);
    b = cc_find<GLOBAL>(P, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(P + a, b);            // parent[a] = min(parent[a], b), b < a: the invariant holds
    if (old == a) return;                           // a was a root: linked
    a = old;                                        // a had been linked meanwhile: unite its new parent with b
  }
}

// ------------------------------------------------------------------------------------------------ 1. tiles in LDS
__global__ __launch_bounds__(CC_TPB) void cc_tile_kernel(const u8* __restrict__ labels, const long long* __restrict__ desc,
                                                         const u8* __restrict__ group, int conn8, int* __restrict__ roots,
                                                         int* __restrict__ area) {
  __shared__ int lab[CC_TW * CC_TH];
  __shared__ u8 g[CC_TH][CC_TW];
  __shared__ u8 lut[256];
  const CcImage im = cc_image(desc, blockIdx.y);
  if (!im.ok) return;
  const int tid = threadIdx.x, tx = (im.W + CC_TW - 1) / CC_TW, ty = (im.H + CC_TH - 1) / CC_TH;
  if ((long long)blockIdx.x >= (long long)tx * ty) return;
  const int x0 = (int)(blockIdx.x % tx) * CC_TW, y0 = (int)(blockIdx.x / tx) * CC_TH;
  const int tw = min(CC_TW, im.W - x0), th = min(CC_TH, im.H - y0);
  const long long HW = (long long)im.H * im.W;
  lut[tid] = group[tid];                                                // CC_TPB == 256: one table entry per thread
  __syncthreads();

  // ---- group ids of the tile: row r is the bytes [s, s + tw); aligned 16-byte windows inside the image span are loaded
  // whole, the others (only around the first and last bytes of an image) byte by byte; nothing outside the span is read
  const uintptr_t span = (uintptr_t)(labels + im.off);
  for (int t = tid; t < CC_TH * CC_CHUNKS; t += CC_TPB) {
    const int r = t / CC_CHUNKS, c = t % CC_CHUNKS;
    if (r >= th) continue;
    const uintptr_t s = span + (uintptr_t)((long long)(y0 + r) * im.W + x0), ca = (s & ~(uintptr_t)15) + 16u * c;
    const uintptr_t lo = ca > s ? ca : s, hi = ca + 16 < s + tw ? ca + 16 : s + tw;
    if (lo >= hi) continue;
    if (ca >= span && ca + 16 <= span + (uintptr_t)HW) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(ca);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uintptr_t a = ca + j;
        if (a >= lo && a < hi) g[r][a - s] = lut[(v[j >> 2] >> (8 * (j & 3))) & 0xffu];
      }
    } else {
      for (uintptr_t a = lo; a < hi; ++a) g[r][a - s] = lut[*reinterpret_cast<const u8*>(a)];
    }
  }
  __syncthreads();

  // ---- a thread's 8 pixels: runs sequentially (the parent of a pixel is the first pixel of its run)
  const int row = tid / (CC_TW / CC_RUN), lx0 = (tid % (CC_TW / CC_RUN)) * CC_RUN;
  const bool live = row < th;
  if (live) {
    int first = row * CC_TW + lx0;
    for (int k = 0; k < CC_RUN && lx0 + k < tw; ++k) {
      const int i = row * CC_TW + lx0 + k;
      if (k > 0 && g[row][lx0 + k] != g[row][lx0 + k - 1]) first = i;
      lab[i] = first;
    }
  }
  __syncthreads();
  // ---- unions with the west / north-west / north / north-east neighbours inside the tile.  Left out where implied:
  // north, when west and north-west are of the same group too (west -- me, north-west -- north, west -- north-west are made
  // by this pixel, by north and, by induction along the row, by west); a diagonal, when north is of the group (north joins
  // both), and north-west when west is (west -- north-west is west's own north)
  if (live) {
    for (int k = 0; k < CC_RUN && lx0 + k < tw; ++k) {
      const int lx = lx0 + k, i = row * CC_TW + lx;
      const u8 me = g[row][lx];
      const bool gW = lx > 0 && g[row][lx - 1] == me;
      if (k == 0 && gW) cc_union<false>(lab, i, i - 1);
      if (row == 0) continue;
      const bool gN = g[row - 1][lx] == me, gNW = lx > 0 && g[row - 1][lx - 1] == me;
      if (gN) {
        if (!(gW && gNW)) cc_union<false>(lab, i, i - CC_TW);
      } else if (conn8) {
        if (gNW && !gW) cc_union<false>(lab, i, i - CC_TW - 1);
        if (lx + 1 < tw && g[row - 1][lx + 1] == me) cc_union<false>(lab, i, i - CC_TW + 1);
      }
    }
  }
  __syncthreads();
  // ---- tile-local roots as image indices (row-major order inside a tile is the image's: the least stays the least)
  if (live) {
    for (int k = 0; k < CC_RUN && lx0 + k < tw; ++k) {
      const int lx = lx0 + k, r = cc_find<false>(lab, row * CC_TW + lx);
      const long long e = im.off + (long long)(y0 + row) * im.W + x0 + lx;
      roots[e] = (y0 + r / CC_TW) * im.W + x0 + r % CC_TW;
      area[e] = 0;
    }
  }
}

// ------------------------------------------------------------------------------------------------ 2. tile borders
__global__ __launch_bounds__(CC_MERGE_TPB) void cc_merge_kernel(const u8* __restrict__ labels, const long long* __restrict__ desc,
                                                                const u8* __restrict__ group, int conn8, int* __restrict__ roots) {
  const CcImage im = cc_image(desc, blockIdx.y);
  if (!im.ok) return;
  const int tid = threadIdx.x, tx = (im.W + CC_TW - 1) / CC_TW, ty = (im.H + CC_TH - 1) / CC_TH;
  if ((long long)blockIdx.x >= (long long)tx * ty) return;
  const int x0 = (int)(blockIdx.x % tx) * CC_TW, y0 = (int)(blockIdx.x / tx) * CC_TH, W = im.W;
  const u8* __restrict__ L = labels + im.off;
  int* P = roots + im.off;
#define CC_G(yy, xx) group[L[(long long)(yy) * W + (xx)]]
  if (tid < CC_TW) {
    // top row: the neighbours of row y0 - 1, with the rules of cc_tile_kernel in image coordinates
    const int x = x0 + tid, y = y0;
    if (y == 0 || x >= W) return;
    const int p = y * W + x;
    const u8 me = CC_G(y, x);
    const bool gW = x > 0 && CC_G(y, x - 1) == me, gN = CC_G(y - 1, x) == me, gNW = x > 0 && CC_G(y - 1, x - 1) == me;
    if (gN) {
      // (never left out at the tile's corner: there west -- me is the left column's union, which may itself be left out
      // BECAUSE north -- me is made here)
      if (!(gW && gNW && tid > 0)) cc_union<true>(P, p, p - W);
    } else if (conn8) {
      if (gNW && !gW) cc_union<true>(P, p, p - W - 1);
      if (x + 1 < W && CC_G(y - 1, x + 1) == me) cc_union<true>(P, p, p - W + 1);
    }
  } else if (tid < CC_TW + CC_TH) {
    // left column: west; the diagonals that cross the vertical border below the tile's first row (through the corner
    // they belong to the top row above): north-west, and south-west, which is the north-east of the pixel left below
    const int ly = tid - CC_TW, x = x0, y = y0 + ly;
    if (x == 0 || y >= im.H) return;
    const int p = y * W + x;
    const u8 me = CC_G(y, x);
    const bool gW = CC_G(y, x - 1) == me, gN = y > 0 && CC_G(y - 1, x) == me, gNW = y > 0 && CC_G(y - 1, x - 1) == me;
    if (gW) {
      // left out when north and north-west are of the group: north -- me and north-west -- west are made elsewhere,
      // north-west -- north by the pixel above, by induction up the column
      if (!(gN && gNW)) cc_union<true>(P, p, p - 1);
    } else if (conn8) {
      if (ly > 0 && gNW && !gN) cc_union<true>(P, p, p - W - 1);
      if (ly < CC_TH - 1 && y + 1 < im.H && CC_G(y + 1, x - 1) == me) cc_union<true>(P, p + W - 1, p);
    }
  }
#undef CC_G
}

// ------------------------------------------------------------------------------------------------ 3. roots and areas
__global__ __launch_bounds__(CC_TPB) void cc_flatten_kernel(const long long* __restrict__ desc, int* __restrict__ roots,
                                                            int* __restrict__ area) {
  __shared__ int block_key;
  __shared__ int block_sum;
  const CcImage im = cc_image(desc, blockIdx.y);
  if (!im.ok) return;
  const int tid = threadIdx.x, lane = tid & (HRSEG_WAVE - 1), tx = (im.W + CC_TW - 1) / CC_TW, ty = (im.H + CC_TH - 1) / CC_TH;
  if ((long long)blockIdx.x >= (long long)tx * ty) return;
  const int x0 = (int)(blockIdx.x % tx) * CC_TW, y0 = (int)(blockIdx.x / tx) * CC_TH;
  const int tw = min(CC_TW, im.W - x0), th = min(CC_TH, im.H - y0);
  int* P = roots + im.off;
  int* A = area + im.off;
  const int row = tid / (CC_TW / CC_RUN), lx0 = (tid % (CC_TW / CC_RUN)) * CC_RUN;
  // a thread's pixels folded into runs of one root: key[j] with cnt[j] pixels, j < n
  int key[CC_RUN], cnt[CC_RUN], n = 0;
#pragma unroll
  for (int k = 0; k < CC_RUN; ++k) key[k] = cnt[k] = 0;
  if (row < th) {
#pragma unroll
    for (int k = 0; k < CC_RUN; ++k) {
      if (lx0 + k >= tw) break;
      const int p = (y0 + row) * im.W + x0 + lx0 + k;
      const int r = cc_find<true>(P, p);
      P[p] = r;                               // (a concurrent walk through p reads the old parent or the root: both are ancestors)
      bool fresh = true;
#pragma unroll
      for (int j = 0; j < CC_RUN; ++j)
        if (j == n - 1 && key[j] == r) {
          cnt[j] += 1;
          fresh = false;
        }
      if (fresh) {
#pragma unroll
        for (int j = 0; j < CC_RUN; ++j)
          if (j == n) {
            key[j] = r;
            cnt[j] = 1;
          }
        n += 1;
      }
    }
  }
  if (tid == 0) {
    block_key = key[0];                       // thread 0 owns the tile's first pixel, which always exists
    block_sum = 0;
  }
  __syncthreads();
  // ---- the block's first root once per block
  const int bk = block_key;
  int mine = 0;
#pragma unroll
  for (int j = 0; j < CC_RUN; ++j)
    if (j < n && key[j] == bk) {
      mine += cnt[j];
      cnt[j] = 0;
    }
  mine = lm_wave_sum(mine);
  if (lane == 0 && mine) atomicAdd(&block_sum, mine);
  // ---- the other roots: once per wave where lanes share one, CC_PEEL rounds per run slot, then every lane for itself
#pragma unroll
  for (int j = 0; j < CC_RUN; ++j) {
    bool has = j < n && cnt[j] > 0;
    u64 todo = __ballot(has);
    for (int it = 0; it < CC_PEEL && todo; ++it) {
      const int leader = __ffsll((long long)todo) - 1;
      const int k = __builtin_amdgcn_readlane(key[j], leader);
      const bool same = has && key[j] == k;
      const int s = lm_wave_sum(same ? cnt[j] : 0);
      if (lane == leader) atomicAdd(&A[k], s);
      has = has && !same;
      todo &= ~__ballot(same);
    }
    if (has) atomicAdd(&A[key[j]], cnt[j]);
  }
  __syncthreads();
  if (tid == 0 && block_sum) atomicAdd(&A[bk], block_sum);
}

// ------------------------------------------------------------------------------------------------ 4. largest per group
__device__ __forceinline__ u64 cc_best_word(int a, int first) { return ((u64)(unsigned)a << 32) | (u64)(0x7fffffffu - (unsigned)first); }

// (a kernel, not a memset: a captured graph must replay the clear in stream order, see ops.zeros)
__global__ __launch_bounds__(CC_TPB) void cc_clear_kernel(u64* __restrict__ best) { best[(size_t)blockIdx.x * 256 + threadIdx.x] = 0; }

__global__ __launch_bounds__(CC_TPB) void cc_best_kernel(const u8* __restrict__ labels, const long long* __restrict__ desc,
                                                         const u8* __restrict__ group, const int* __restrict__ area,
                                                         u64* __restrict__ best) {
  __shared__ u64 sbest[256];
  const CcImage im = cc_image(desc, blockIdx.y);
  if (!im.ok) return;
  const long long HW = (long long)im.H * im.W, i0 = ((long long)blockIdx.x * CC_TPB + threadIdx.x) * CC_BEST_STEP;
  if ((long long)blockIdx.x * CC_TPB * CC_BEST_STEP >= HW) return;
  sbest[threadIdx.x] = 0;
  __syncthreads();
  for (int k = 0; k < CC_BEST_STEP; ++k) {
    const long long i = i0 + k;
    if (i >= HW) break;
    const int a = area[im.off + i];
    if (a > 0) atomicMax(&sbest[group[labels[im.off + i]]], cc_best_word(a, (int)i));
  }
  __syncthreads();
  const u64 v = sbest[threadIdx.x];
  if (v) atomicMax(&best[(size_t)blockIdx.y * 256 + threadIdx.x], v);
}

// ------------------------------------------------------------------------------------------------ 5. filter
struct CcRule {
  int min_area, keep_largest, fill;
};

__global__ __launch_bounds__(CC_TPB) void cc_filter_kernel(const u8* __restrict__ labels, const long long* __restrict__ desc,
                                                           const u8* __restrict__ group, const CcRule* __restrict__ rules,
                                                           const int* __restrict__ roots, const int* __restrict__ area,
                                                           const u64* __restrict__ best, u8* __restrict__ out,
                                                           u64* __restrict__ stats) {
  __shared__ unsigned hist[256 * 3];
  const CcImage im = cc_image(desc, blockIdx.y);
  if (!im.ok) return;
  const long long HW = (long long)im.H * im.W;
  const u8* __restrict__ L = labels + im.off;
  const int* __restrict__ R = roots + im.off;
  const int* __restrict__ A = area + im.off;
  u8* __restrict__ O = out + im.off;
  const int mis = (int)((uintptr_t)L & (CC_STEP - 1));                   // L - mis is 16-byte aligned
  if ((long long)blockIdx.x * CC_TPB * CC_STEP >= HW + mis) return;
  for (int i = threadIdx.x; i < 256 * 3; i += CC_TPB) hist[i] = 0;
  __syncthreads();
  const long long i0 = ((long long)blockIdx.x * CC_TPB + threadIdx.x) * CC_STEP - mis;
  if (i0 < HW && i0 + CC_STEP > 0) {
    unsigned v[4];
    const bool whole = i0 >= 0 && i0 + CC_STEP <= HW;
    if (whole) {
      const u32x4 t = *reinterpret_cast<const u32x4*>(L + i0);           // L + i0 is 16-byte aligned
      v[0] = t[0], v[1] = t[1], v[2] = t[2], v[3] = t[3];
    } else {
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        v[d] = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const long long i = i0 + 4 * d + j;
          if (i >= 0 && i < HW) v[d] |= (unsigned)L[i] << (8 * j);
        }
      }
    }
    unsigned o[4] = {v[0], v[1], v[2], v[3]};
    int last_root = -1, last_g = 0;
    bool last_removed = false;
    unsigned last_fill = 0, npix = 0;
#pragma unroll
    for (int e = 0; e < CC_STEP; ++e) {
      const long long i = i0 + e;
      if (i < 0 || i >= HW) continue;
      const int r = R[i];
      if (r != last_root) {
        if (npix) atomicAdd(&hist[last_g * 3 + 2], npix);
        npix = 0;
        last_root = r;
        last_g = group[L[r]];
        last_removed = false;
        if (last_g != 255) {
          const CcRule rule = rules[last_g];
          const int a = A[r];
          bool rem = a < rule.min_area;
          if (rule.keep_largest && (unsigned)(best[(size_t)blockIdx.y * 256 + last_g] & 0xffffffffu) != 0x7fffffffu - (unsigned)r) rem = true;
          if (rem) {
            if (rule.fill >= 0) {
              last_fill = (unsigned)rule.fill & 0xffu;
              last_removed = true;
            } else if (r % im.W > 0) {
              last_fill = L[r - 1];
              last_removed = true;
            } else if (r >= im.W) {
              last_fill = L[r - im.W];
              last_removed = true;
            }                                                            // the image's origin: the component stays
          }
        }
      }
      if ((long long)r == i) {
        atomicAdd(&hist[last_g * 3], 1u);
        if (last_removed) atomicAdd(&hist[last_g * 3 + 1], 1u);
      }
      if (last_removed) {
        npix += 1;
        o[e >> 2] = (o[e >> 2] & ~(0xffu << (8 * (e & 3)))) | (last_fill << (8 * (e & 3)));
      }
    }
    if (npix) atomicAdd(&hist[last_g * 3 + 2], npix);
    if (whole && ((uintptr_t)(O + i0) & 15) == 0) {
      u32x4 t;
      t[0] = o[0], t[1] = o[1], t[2] = o[2], t[3] = o[3];
      *reinterpret_cast<u32x4*>(O + i0) = t;
    } else {
#pragma unroll
      for (int e = 0; e < CC_STEP; ++e) {
        const long long i = i0 + e;
        if (i >= 0 && i < HW) O[i] = (u8)(o[e >> 2] >> (8 * (e & 3)));
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 256 * 3; i += CC_TPB)
    if (hist[i]) atomicAdd(&stats[(size_t)blockIdx.y * 768 + i], (u64)hist[i]);
}

// ------------------------------------------------------------------------------------------------------------ C ABI
// the host copy of the descriptors, every row acceptable to lm_host_image (labelmap_common.h: H*W < 2^31) -> tiles and
// pixels of the largest image, bytes spanned
static int cc_scan(const char* who, const long* desc_host, int B, long long* max_tiles, long long* max_hw, long long* extent) {
  *max_tiles = *max_hw = *extent = 0;
  for (int b = 0; b < B; ++b) {
    long long off, H, W;
    if (int rc = lm_host_image(who, "", desc_host, b, &off, &H, &W)) return rc;
    const long long tiles = ((W + CC_TW - 1) / CC_TW) * ((H + CC_TH - 1) / CC_TH);
    *max_tiles = tiles > *max_tiles ? tiles : *max_tiles;
    *max_hw = H * W > *max_hw ? H * W : *max_hw;
    *extent = off + H * W > *extent ? off + H * W : *extent;
  }
  return 0;
}

extern "C" int hrseg_components_tile(int* w, int* h) {
  HRSEG_CHECK_ARG(w && h, "hrseg_components_tile: null pointer");
  *w = CC_TW;
  *h = CC_TH;
  return 0;
}

extern "C" size_t hrseg_filter_components_workspace_bytes(int B) { return B > 0 ? (size_t)B * 256 * sizeof(u64) : 0; }

extern "C" int hrseg_label_components(const unsigned char* labels, const long* desc, const long* desc_host, int B,
                                      const unsigned char* group, int connectivity, int* roots, int* area, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(labels && desc && desc_host && group && roots && area, "hrseg_label_components: null pointer");
  HRSEG_CHECK_ARG(B >= 1 && B <= 65535, "hrseg_label_components: B=%d not in 1..65535", B);
  HRSEG_CHECK_ARG(connectivity == 4 || connectivity == 8, "hrseg_label_components: connectivity %d, supported 4 and 8", connectivity);
  HRSEG_CHECK_ARG(((uintptr_t)roots & 3) == 0 && ((uintptr_t)area & 3) == 0, "hrseg_label_components: roots and area must be 4-byte aligned");
  long long tiles, hw, extent;
  if (int rc = cc_scan("hrseg_label_components", desc_host, B, &tiles, &hw, &extent)) return rc;
  const dim3 grid((unsigned)tiles, (unsigned)B);
  const int conn8 = connectivity == 8;
  hipLaunchKernelGGL(cc_tile_kernel, grid, dim3(CC_TPB), 0, (hipStream_t)stream, labels, (const long long*)desc, group, conn8, roots, area);
  HRSEG_LAUNCH_CHECK("label_components (tiles)");
  hipLaunchKernelGGL(cc_merge_kernel, grid, dim3(CC_MERGE_TPB), 0, (hipStream_t)stream, labels, (const long long*)desc, group, conn8, roots);
  HRSEG_LAUNCH_CHECK("label_components (merge)");
  hipLaunchKernelGGL(cc_flatten_kernel, grid, dim3(CC_TPB), 0, (hipStream_t)stream, (const long long*)desc, roots, area);
  HRSEG_LAUNCH_CHECK("label_components (flatten)");
  hrseg_count(CNT_LABEL_COMPONENTS, HRSEG_LABEL_COMPONENTS_LAUNCHES);
  return 0;
}

extern "C" int hrseg_filter_components(const unsigned char* labels, const long* desc, const long* desc_host, int B,
                                       const unsigned char* group, const hrseg_component_rule_t* rules, const int* roots,
                                       const int* area, unsigned char* out, long long* stats, void* workspace,
                                       hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(labels && desc && desc_host && group && rules && roots && area && out && stats && workspace,
                  "hrseg_filter_components: null pointer");
  HRSEG_CHECK_ARG(B >= 1 && B <= 65535, "hrseg_filter_components: B=%d not in 1..65535", B);
  HRSEG_CHECK_ARG(((uintptr_t)roots & 3) == 0 && ((uintptr_t)area & 3) == 0 && ((uintptr_t)rules & 3) == 0,
                  "hrseg_filter_components: roots, area and rules must be 4-byte aligned");
  HRSEG_CHECK_ARG(((uintptr_t)stats & 7) == 0 && ((uintptr_t)workspace & 7) == 0,
                  "hrseg_filter_components: stats and workspace must be 8-byte aligned");
  long long tiles, hw, extent;
  if (int rc = cc_scan("hrseg_filter_components", desc_host, B, &tiles, &hw, &extent)) return rc;
  HRSEG_CHECK_ARG((uintptr_t)out + (uintptr_t)extent <= (uintptr_t)labels || (uintptr_t)labels + (uintptr_t)extent <= (uintptr_t)out,
                  "hrseg_filter_components: out overlaps labels");
  static_assert(sizeof(hrseg_component_rule_t) == sizeof(CcRule), "the kernel reads the rules as three ints");
  hipLaunchKernelGGL(cc_clear_kernel, dim3((unsigned)B), dim3(CC_TPB), 0, (hipStream_t)stream, (u64*)workspace);
  HRSEG_LAUNCH_CHECK("filter_components (clear)");
  const unsigned best_steps = (unsigned)((hw + CC_TPB * CC_BEST_STEP - 1) / (CC_TPB * CC_BEST_STEP));
  hipLaunchKernelGGL(cc_best_kernel, dim3(best_steps, (unsigned)B), dim3(CC_TPB), 0, (hipStream_t)stream, labels, (const long long*)desc,
                     group, area, (u64*)workspace);
  HRSEG_LAUNCH_CHECK("filter_components (largest)");
  const unsigned steps = (unsigned)((hw + (CC_STEP - 1) + CC_TPB * CC_STEP - 1) / (CC_TPB * CC_STEP));
  hipLaunchKernelGGL(cc_filter_kernel, dim3(steps, (unsigned)B), dim3(CC_TPB), 0, (hipStream_t)stream, labels, (const long long*)desc, group,
                     (const CcRule*)rules, roots, area, (const u64*)workspace, out, (u64*)stats);
  HRSEG_LAUNCH_CHECK("filter_components (filter)");
  hrseg_count(CNT_FILTER_COMPONENTS, HRSEG_FILTER_COMPONENTS_LAUNCHES);
  return 0;
}
