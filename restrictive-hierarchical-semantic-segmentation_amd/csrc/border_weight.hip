// Border weight maps (include/hrseg.h, "border weights"): a level's ternary target planes [B,C,H,W] ->
// the label map (one byte per pixel), the squared distance d2 of every pixel to the nearest pixel of another label within
// `radius`, and v = lut[d2].  gfx950.  Integer arithmetic up to the table lookup: the same bytes in every run.
//
//   1. bw_labels_kernel: a thread owns a pixel and reads its C channels one plane at a time (a wave reads 256 contiguous
//      bytes of each plane); label = the first channel that is 1, C when none is, 255 when every channel is -1 (void).
//   2. bw_search_kernel: a block owns a BW_TW x BW_TH tile.  It stages the tile's label bytes plus a halo (radius rows above and
//      below, radius + 6 columns rounded up to a dword on either side; 255 outside the frame) in LDS as dwords and notes
//      which labels each staged row and the whole window hold.  A window with at most one non-void label is done at once
//      (d2 = 0 everywhere: background, jaw, the inside of large regions).  Otherwise a wave owns a tile row, a lane a pixel:
//      rows by increasing |dy| until dy^2 >= best, skipping the rows that hold nothing but the pixel's own label and void; in a
//      row the dword of the pixel, then pairs of dwords outwards (four labels per LDS read, compared as bytes in a register)
//      as far as best allows.  The four lanes of a dword read the same address (a broadcast) and a wave reads consecutive
//      dwords: no bank conflicts.
#include "labelmap_common.h"
#include "level_common.h"

#define BW_TW HRSEG_BORDER_TILE_W
#define BW_TH HRSEG_BORDER_TILE_H
#define BW_TPB 256
#define BW_MAXR HRSEG_BORDER_MAX_RADIUS
#define BW_HALO_X(R) (((R) + 9) & ~3)                    // >= R + 6: the outermost dword pair a search may touch
#define BW_ROWS (BW_TH + 2 * BW_MAXR)
#define BW_STRIDE_DW ((BW_TW + 2 * BW_HALO_X(BW_MAXR)) / 4)
static_assert(BW_TW == 64 && BW_TPB == 4 * BW_TW && BW_TH % 4 == 0, "a wave owns a tile row, a lane a pixel");
static_assert(MAXC == 16 && BW_MAXR * BW_MAXR + 1 < (1 << 30), "labels 0..16 are bits of a 32-bit set");

__global__ __launch_bounds__(256) void bw_labels_kernel(const float* __restrict__ t, u8* __restrict__ labels, int C, long hw,
                                                        long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long b = i / hw, pix = i - b * hw;
    const float* tb = t + (size_t)b * C * hw + pix;
    int lab = C;
    bool all_void = true;
#pragma unroll 4
    for (int c = C - 1; c >= 0; --c) {
      const float v = tb[(size_t)c * hw];
      if (v == 1.f) lab = c;
      if (v != -1.f) all_void = false;       // (NaN: not on, not -1)
    }
    labels[i] = all_void ? (u8)255 : (u8)lab;
  }
}

// bit 7 of every byte of x that is not 0
__device__ __forceinline__ u32 bw_nonzero_bytes(u32 x) { return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u; }
// the bytes of w that are a source for a pixel of label L (lrep = L in every byte): another label, and not void
__device__ __forceinline__ u32 bw_sources(u32 w, u32 lrep) { return bw_nonzero_bytes(w ^ lrep) & bw_nonzero_bytes(~w); }

__global__ __launch_bounds__(BW_TPB) void bw_search_kernel(const u8* __restrict__ labels, const float* __restrict__ lut,
                                                           float* __restrict__ v, int* __restrict__ d2, int H, int W, int R,
                                                           int tx, int ty, long total, int aligned) {
  __shared__ u32 tile[BW_ROWS * BW_STRIDE_DW];
  __shared__ u32 rowmask[BW_ROWS];          // the labels a staged row holds, as a bit set (void has no bit)
  __shared__ u32 seen;                      // ... the whole window
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int hx = BW_HALO_X(R), sdw = (BW_TW + 2 * hx) >> 2, rows = BW_TH + 2 * R;
  for (long id = blockIdx.x; id < total; id += gridDim.x) {
    const int b = (int)(id / ((long)tx * ty)), rem = (int)(id - (long)b * tx * ty);
    const int x0 = (rem % tx) * BW_TW, y0 = (rem / tx) * BW_TH;
    const u8* img = labels + (size_t)b * H * W;
    __syncthreads();                        // the readers of the tile before this one are done
    for (int r = tid; r < rows; r += BW_TPB) rowmask[r] = 0;
    if (tid == 0) seen = 0;
    __syncthreads();
    u32 mine = 0;
    for (int e = tid; e < rows * sdw; e += BW_TPB) {
      const int r = e / sdw, cdw = e - r * sdw;
      const int gy = y0 - R + r, gx = x0 - hx + 4 * cdw;
      u32 w = 0xffffffffu;
      if (gy >= 0 && gy < H && gx + 3 >= 0 && gx < W) {
        const u8* p = img + (size_t)gy * W;
        if (aligned && gx >= 0 && gx + 3 < W) {
          w = *(const u32*)(p + gx);
        } else {
          w = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int x = gx + j;
            w |= ((x >= 0 && x < W) ? (u32)p[x] : 255u) << (8 * j);
          }
        }
      }
      tile[r * sdw + cdw] = w;
      u32 m = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u32 l = (w >> (8 * j)) & 255u;
        if (l <= MAXC) m |= 1u << l;
      }
      if (m) atomicOr(&rowmask[r], m);
      mine |= m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine |= (u32)__shfl_xor((int)mine, o, 64);
    if (lane == 0 && mine) atomicOr(&seen, mine);
    __syncthreads();
    const u32 all = seen;
    const bool uniform = __popc(all) <= 1;  // the same in every lane of the block: the early-out
    const int gx = x0 + lane;
#pragma unroll 1
    for (int k = 0; k < BW_TH / 4; ++k) {
      const int ly = wv + 4 * k, gy = y0 + ly;
      if (gy >= H || gx >= W) continue;
      int best = 0;
      if (!uniform) {
        const int cy = R + ly, cx = hx + lane, xo = cx & 3, cdw = cx >> 2;
        const u32 L = (tile[cy * sdw + cdw] >> (8 * xo)) & 255u;
        if (L != 255u && (all & ~(1u << L))) {
          const u32 lrep = L * 0x01010101u, others = ~(1u << L);
          int bv = R * R + 1;
          for (int dy = 0; dy <= R; ++dy) {
            const int dy2 = dy * dy;
            if (dy2 >= bv) break;
            for (int s = 0; s < (dy ? 2 : 1); ++s) {
              const int r = s ? cy + dy : cy - dy;
              if (!(rowmask[r] & others)) continue;
              const u32* row = tile + r * sdw + cdw;
              const u32 mc = bw_sources(row[0], lrep);
              if (mc) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                  if (mc & (0x80u << (8 * j))) bv = min(bv, (j - xo) * (j - xo) + dy2);
              }
              for (int q = 1;; ++q) {       // the dwords q to the left and to the right: |dx| >= 4q - 3 in both
                const int lo = 4 * q - 3;
                if (lo * lo + dy2 >= bv) break;
                const u32 mr = bw_sources(row[q], lrep), ml = bw_sources(row[-q], lrep);
                if (mr) {
                  const int dx = 4 * q - xo + ((__ffs((int)mr) - 1) >> 3);
                  bv = min(bv, dx * dx + dy2);
                }
                if (ml) {
                  const int dx = 4 * q + xo - ((31 - __clz((int)ml)) >> 3);
                  bv = min(bv, dx * dx + dy2);
                }
              }
            }
          }
          best = bv > R * R ? 0 : bv;
        }
      }
      const size_t o = (size_t)b * H * W + (size_t)gy * W + gx;
      v[o] = lut[best];
      if (d2) d2[o] = best;
    }
  }
}

extern "C" int hrseg_border_tile(int* w, int* h) {
  HRSEG_CHECK_ARG(w && h, "hrseg_border_tile: null pointer");
  *w = BW_TW;
  *h = BW_TH;
  return 0;
}

extern "C" int hrseg_border_weights(const float* t, int B, int C, int H, int W, int radius, const float* lut,
                                    unsigned char* labels, float* v, int* d2, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(t && lut && labels && v, "hrseg_border_weights: null pointer (t, lut, labels, v)");
  HRSEG_CHECK_ARG(B >= 1 && C >= 1 && C <= MAXC && H >= 1 && W >= 1, "hrseg_border_weights: bad arguments (B=%d, C=%d, %d x %d)", B, C,
                  H, W);
  HRSEG_CHECK_ARG((long long)H * W < (1ll << 31), "hrseg_border_weights: %d x %d has 2^31 pixels or more", H, W);
  HRSEG_CHECK_ARG(radius >= 1 && radius <= BW_MAXR, "hrseg_border_weights: radius %d outside 1..%d", radius, BW_MAXR);
  hipStream_t st = (hipStream_t)stream;
  const long hw = (long)H * W, n = (long)B * hw;
  hipLaunchKernelGGL(bw_labels_kernel, dim3(pixel_blocks(n, 4096)), dim3(256), 0, st, t, labels, C, hw, n);
  const int tx = ceil_div(W, BW_TW), ty = ceil_div(H, BW_TH);
  const long total = (long)B * tx * ty;
  const int aligned = (W % 4 == 0) && ((uintptr_t)labels % 4 == 0);
  hipLaunchKernelGGL(bw_search_kernel, dim3((unsigned)(total < (1l << 20) ? total : (1l << 20))), dim3(BW_TPB), 0, st,
                     (const u8*)labels, lut, v, d2, H, W, radius, tx, ty, total, aligned);
  hrseg_count(CNT_BORDER_WEIGHTS, 2);
  HRSEG_LAUNCH_CHECK("hrseg_border_weights");
  return 0;
}
