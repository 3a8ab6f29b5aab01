// Pooling, bilinear resize, the HRNet fuse sum and elementwise glue on NHWC fp32 for gfx950.  All HBM-bound: one pass
// per tensor, 16-byte accesses.  Thread mapping: elem_common.h.
#include "elem_common.h"

// --------------------------------------------------------------------------- max pool 2x2 (floor)
__global__ __launch_bounds__(256) void maxpool2_fwd_kernel(const float* __restrict__ x, int ldx,
                                                           float* __restrict__ y, int ldy, int B, int Hi, int Wi,
                                                           int C) {
  const Lanes L = make_lanes(C);
  if (!L.active) return;
  const int Ho = Hi / 2, Wo = Wi / 2;
  const long npix = (long)B * Ho * Wo;
  FOR_PIXELS(pix, L, npix) {
    const int b = (int)(pix / ((long)Ho * Wo));
    const int rem = (int)(pix - (long)b * Ho * Wo);
    const int oy = rem / Wo, ox = rem - oy * Wo;
    const float* p = x + (((size_t)b * Hi + 2 * oy) * Wi + 2 * ox) * ldx + 4 * L.cq;
    f32x4 m = ld4(p);
    const f32x4 v1 = ld4(p + ldx), v2 = ld4(p + (size_t)Wi * ldx), v3 = ld4(p + (size_t)Wi * ldx + ldx);
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = max_nan(max_nan(m[j], v1[j]), max_nan(v2[j], v3[j]));   // NaN in the window -> NaN, as torch
    st4(y + pix * ldy + 4 * L.cq, m);
  }
}

// gradient goes to the first maximum in scan order (strict >), as torch's max_pool2d
__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(const float* __restrict__ x, int ldx,
                                                           const float* __restrict__ dy, int lddy,
                                                           float* __restrict__ dx, int lddx, int acc, int B,
                                                           int Hi, int Wi, int C) {
  const Lanes L = make_lanes(C);
  if (!L.active) return;
  const int Hc = (Hi + 1) / 2, Wc = (Wi + 1) / 2;  // cells incl. the odd leftover row/col
  const int Ho = Hi / 2, Wo = Wi / 2;
  const long ncell = (long)B * Hc * Wc;
  FOR_PIXELS(cell, L, ncell) {
    const int b = (int)(cell / ((long)Hc * Wc));
    const int rem = (int)(cell - (long)b * Hc * Wc);
    const int oy = rem / Wc, ox = rem - oy * Wc;
    const size_t base = (((size_t)b * Hi + 2 * oy) * Wi + 2 * ox);
    const bool full = (oy < Ho) & (ox < Wo);
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    int arg[4] = {-1, -1, -1, -1};
    if (full) {
      g = ld4(dy + (((size_t)b * Ho + oy) * Wo + ox) * lddy + 4 * L.cq);
      f32x4 m = ld4(x + base * ldx + 4 * L.cq);
#pragma unroll
      for (int j = 0; j < 4; ++j) arg[j] = 0;
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        const f32x4 v = ld4(x + (base + (k >> 1) * Wi + (k & 1)) * ldx + 4 * L.cq);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (v[j] > m[j]) { m[j] = v[j]; arg[j] = k; }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int iy = 2 * oy + (k >> 1), ix = 2 * ox + (k & 1);
      if (iy >= Hi || ix >= Wi) continue;
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (arg[j] == k) ? g[j] : 0.f;
      float* d = dx + (base + (k >> 1) * Wi + (k & 1)) * lddx + 4 * L.cq;
      st4(d, acc ? ld4(d) + o : o);
    }
  }
}

// --------------------------------------------------------------------------- bilinear
// source coordinate exactly as torch's upsample_bilinear2d (fp32 arithmetic)
__device__ __forceinline__ void src_index(int o, float scale, int in_size, int align, int& i0, int& i1,
                                          float& l0, float& l1) {
  float r;
  if (align) {
    r = scale * (float)o;
  } else {
    r = scale * ((float)o + 0.5f) - 0.5f;
    if (r < 0.f) r = 0.f;
  }
  i0 = (int)r;
  if (i0 > in_size - 1) i0 = in_size - 1;
  i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
  l1 = r - (float)i0;
  l0 = 1.f - l1;
}
static float resize_scale(int in_size, int out_size, int align) {
  if (align) return out_size > 1 ? (float)(in_size - 1) / (float)(out_size - 1) : 0.f;
  return (float)in_size / (float)out_size;
}

__global__ __launch_bounds__(256) void bilinear_fwd_kernel(const float* __restrict__ in, int ldin, int B, int Hi,
                                                           int Wi, int C, float* __restrict__ out, int ldout,
                                                           int Hout, int Wout, int Hr, int Wr, int py, int px,
                                                           float sh, float sw, int align, int acc, int relu) {
  const Lanes L = make_lanes(C);
  if (!L.active) return;
  const long npix = (long)B * Hout * Wout;
  FOR_PIXELS(pix, L, npix) {
    const int b = (int)(pix / ((long)Hout * Wout));
    const int rem = (int)(pix - (long)b * Hout * Wout);
    const int oy = rem / Wout - py, ox = rem % Wout - px;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (oy >= 0 && oy < Hr && ox >= 0 && ox < Wr) {
      int y0, y1, x0, x1;
      float ly0, ly1, lx0, lx1;
      src_index(oy, sh, Hi, align, y0, y1, ly0, ly1);
      src_index(ox, sw, Wi, align, x0, x1, lx0, lx1);
      const float* p = in + (size_t)b * Hi * Wi * ldin + 4 * L.cq;
      const f32x4 v00 = ld4(p + ((size_t)y0 * Wi + x0) * ldin), v01 = ld4(p + ((size_t)y0 * Wi + x1) * ldin);
      const f32x4 v10 = ld4(p + ((size_t)y1 * Wi + x0) * ldin), v11 = ld4(p + ((size_t)y1 * Wi + x1) * ldin);
      v = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
    }
    float* o = out + pix * ldout + 4 * L.cq;
    if (acc) v += ld4(o);
    if (relu) v = relu_nan(v);
    st4(o, v);
  }
}

// HRNet fuse sum (Models/models.py:527-542) in ONE pass: out = relu?( sum of same-resolution terms + sum of bilinearly
// up-sampled low-resolution terms ).  The chain of add / copy / accumulating-bilinear launches it replaces re-reads and
// re-writes `out` once per term.
struct FuseSumArgs {
  int n_same, n_low;
  const float* same[4]; int ld_same[4];
  const float* low[3]; int ld_low[3]; int Hi[3], Wi[3];
  float sh[3], sw[3];
  float* out; int ldo;
  int B, H, W, C, align, relu;
};
__global__ __launch_bounds__(256) void fuse_sum_kernel(FuseSumArgs a) {
  const Lanes L = make_lanes(a.C);
  if (!L.active) return;
  const long npix = (long)a.B * a.H * a.W;
  FOR_PIXELS(pix, L, npix) {
    f32x4 v = ld4(a.same[0] + pix * a.ld_same[0] + 4 * L.cq);
#pragma unroll
    for (int i = 1; i < 4; ++i)
      if (i < a.n_same) v += ld4(a.same[i] + pix * a.ld_same[i] + 4 * L.cq);
    if (a.n_low) {
      const int b = (int)(pix / ((long)a.H * a.W));
      const int rem = (int)(pix - (long)b * a.H * a.W);
      const int oy = rem / a.W, ox = rem - oy * a.W;
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (j < a.n_low) {
          int y0, y1, x0, x1;
          float ly0, ly1, lx0, lx1;
          src_index(oy, a.sh[j], a.Hi[j], a.align, y0, y1, ly0, ly1);
          src_index(ox, a.sw[j], a.Wi[j], a.align, x0, x1, lx0, lx1);
          const int ld = a.ld_low[j], Wi = a.Wi[j];
          const float* p = a.low[j] + (size_t)b * a.Hi[j] * Wi * ld + 4 * L.cq;
          const f32x4 v00 = ld4(p + ((size_t)y0 * Wi + x0) * ld), v01 = ld4(p + ((size_t)y0 * Wi + x1) * ld);
          const f32x4 v10 = ld4(p + ((size_t)y1 * Wi + x0) * ld), v11 = ld4(p + ((size_t)y1 * Wi + x1) * ld);
          v += ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
        }
    }
    if (a.relu) v = relu_nan(v);
    st4(a.out + pix * a.ldo + 4 * L.cq, v);
  }
}

// HRNet head at branch resolution (hrseg_head_mix): y = t0 + sum_j up(t_j) + bias in place over t0, where t_j = W_j x_j are
// the 1x1 convolutions of the branches at their own resolution -- bilinear weights do not depend on the channel and sum to
// one, so the resize commutes with the 1x1 convolution.  fuse_sum_kernel's interpolation expression, the bias added last.
// One block per pixel chunk (stats_body's chunk -> pixel range rule), threads = channel quads x `lanes` pixel lanes (up to
// 1024 threads: a lane's walk is a chain of dependent loads, so the lanes are what keeps bytes in flight); a lane walks its
// piece of the chunk in ascending order and keeps the fp32 sums of y and y^2, the block adds its lanes in lane order in fp64
// and leaves row `chunk` of the [nchunks][2][C] partial sums the BatchNorm finalize phase reads: no atomics, the same bits
// every run, and no statistics pass over y.
struct HeadMixArgs {
  float* y; int ldy;
  const float* bias;
  int n_low;
  const float* low[3]; int ld_low[3]; int Hi[3], Wi[3];
  float sh[3], sw[3];
  int B, H, W, C, align, lanes;
  double* partial; int nchunks;
};
static int head_mix_lanes(int C) { const int p = 1024 / (C / 4); return p > 16 ? 16 : p; }      // (ops.head_mix sizes nchunks by it)
__global__ __launch_bounds__(1024) void head_mix_kernel(HeadMixArgs a) {
  __shared__ float red[1024 * 8];
  Lanes L;
  L.Q = a.C >> 2; L.P = a.lanes; L.cq = threadIdx.x % L.Q; L.pl = threadIdx.x / L.Q; L.active = L.pl < L.P;
  const long npix = (long)a.B * a.H * a.W;
  const long per = (npix + a.nchunks - 1) / a.nchunks;
  const long lo = (long)blockIdx.x * per;
  const long hi = (lo + per < npix) ? lo + per : npix;
  f32x4 s = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
  if (L.active) {
    f32x4 bias = {0.f, 0.f, 0.f, 0.f};
    if (a.bias) bias = ld4(a.bias + 4 * L.cq);
    // A pixel lane walks a contiguous piece of the chunk, left to right along the image rows, and keeps the two columns
    // (x0, x1) x two rows (y0, y1) of every low-resolution term in registers: at a 2x .. 8x resize the next pixel needs the
    // same columns or one new one, so a pixel costs 1.75 low-resolution loads on average instead of 12 (re-reads that would
    // come from beyond L2: the pass would be bound by them, not by HBM)
    const long len = (hi - lo + L.P - 1) / L.P;
    const long p0 = lo + (long)L.pl * len, p1 = (p0 + len < hi) ? p0 + len : hi;
    int cb[3], cy0[3], cy1[3], cxa[3], cxb[3];
    f32x4 ca0[3], ca1[3], cb0[3], cb1[3];            // rows y0 / y1 of column xa, of column xb
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      cb[j] = cy0[j] = cy1[j] = cxa[j] = cxb[j] = -1;
      ca0[j] = ca1[j] = cb0[j] = cb1[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    f32x4 nxt = {0.f, 0.f, 0.f, 0.f};
    if (p0 < p1) nxt = ld4(a.y + p0 * a.ldy + 4 * L.cq);
    for (long pix = p0; pix < p1; ++pix) {
      float* o = a.y + pix * a.ldy + 4 * L.cq;
      f32x4 v = nxt;
      if (pix + 1 < p1) nxt = ld4(o + a.ldy);        // the next pixel's t0 is in flight across this pixel's arithmetic
      const int b = (int)(pix / ((long)a.H * a.W));
      const int rem = (int)(pix - (long)b * a.H * a.W);
      const int oy = rem / a.W, ox = rem - oy * a.W;
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (j < a.n_low) {
          int y0, y1, x0, x1;
          float ly0, ly1, lx0, lx1;
          src_index(oy, a.sh[j], a.Hi[j], a.align, y0, y1, ly0, ly1);
          src_index(ox, a.sw[j], a.Wi[j], a.align, x0, x1, lx0, lx1);
          const int ld = a.ld_low[j], Wi = a.Wi[j];
          const float* p = a.low[j] + (size_t)b * a.Hi[j] * Wi * ld + 4 * L.cq;
          if (b != cb[j] || y0 != cy0[j] || y1 != cy1[j]) {
            cb[j] = b; cy0[j] = y0; cy1[j] = y1;
            cxa[j] = cxb[j] = -1;
          }
          if (x0 != cxa[j]) {
            if (x0 == cxb[j]) {
              ca0[j] = cb0[j]; ca1[j] = cb1[j];
            } else {
              ca0[j] = ld4(p + ((size_t)y0 * Wi + x0) * ld);
              ca1[j] = ld4(p + ((size_t)y1 * Wi + x0) * ld);
            }
            cxa[j] = x0;
          }
          if (x1 != cxb[j]) {
            if (x1 == cxa[j]) {
              cb0[j] = ca0[j]; cb1[j] = ca1[j];
            } else {
              cb0[j] = ld4(p + ((size_t)y0 * Wi + x1) * ld);
              cb1[j] = ld4(p + ((size_t)y1 * Wi + x1) * ld);
            }
            cxb[j] = x1;
          }
          v += ly0 * (lx0 * ca0[j] + lx1 * cb0[j]) + ly1 * (lx0 * ca1[j] + lx1 * cb1[j]);
        }
      v += bias;
      st4(o, v);
      s += v;
      s2 += v * v;
    }
  }
  if (!a.partial) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    red[threadIdx.x * 8 + j] = s[j];
    red[threadIdx.x * 8 + 4 + j] = s2[j];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < a.C; c += blockDim.x) {
    double sa = 0.0, sb = 0.0;
    for (int pl = 0; pl < L.P; ++pl) {
      const int t = pl * L.Q + (c >> 2);
      sa += red[t * 8 + (c & 3)];
      sb += red[t * 8 + 4 + (c & 3)];
    }
    a.partial[((size_t)blockIdx.x * 2 + 0) * a.C + c] = sa;
    a.partial[((size_t)blockIdx.x * 2 + 1) * a.C + c] = sb;
  }
}

// gather form of the transpose: every input pixel sums the output pixels that read it (no atomics,
// deterministic).  An 8x resize gives each input pixel an ~18x18 footprint and only a few thousand input
// pixels: RS sub-lanes per pixel split the footprint rows (thread = channel quad x pixel lane x row split)
// and reduce through LDS, so the small tensors still fill the machine.
template <int RS>
__global__ __launch_bounds__(256) void bilinear_bwd_kernel(const float* __restrict__ dout, int lddout, int B,
                                                           int Hi, int Wi, int C, float* __restrict__ din,
                                                           int lddin, int Hout, int Wout, int Hr, int Wr, int py,
                                                           int px, float sh, float sw, int align, int acc) {
  __shared__ f32x4 red[256];
  const int Q = C >> 2;
  const int P2 = max(1, 256 / (Q * RS));           // pixel lanes per block
  const int cq = threadIdx.x % Q, pl = (threadIdx.x / Q) % P2, rs = threadIdx.x / (Q * P2);
  const bool active = rs < RS && (int)threadIdx.x < Q * P2 * RS;
  const long npix = (long)B * Hi * Wi;
  const float ish = sh > 0.f ? 1.f / sh : 0.f, isw = sw > 0.f ? 1.f / sw : 0.f;
  for (long base = (long)blockIdx.x * P2; base < npix; base += (long)gridDim.x * P2) {
    const long pix = base + pl;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (active && pix < npix) {
      const int b = (int)(pix / ((long)Hi * Wi));
      const int rem = (int)(pix - (long)b * Hi * Wi);
      const int iy = rem / Wi, ix = rem - iy * Wi;
      // candidate output rows/cols: src in (iy-1, iy+1)  (whole range when scale is 0)
      int oy_lo = 0, oy_hi = Hr - 1, ox_lo = 0, ox_hi = Wr - 1;
      if (sh > 0.f) {
        oy_lo = max(0, (int)floorf(((float)iy - 1.f + (align ? 0.f : 0.5f)) * ish - (align ? 0.f : 0.5f)) - 1);
        oy_hi = min(Hr - 1, (int)ceilf(((float)iy + 1.f + (align ? 0.f : 0.5f)) * ish - (align ? 0.f : 0.5f)) + 1);
      }
      if (sw > 0.f) {
        ox_lo = max(0, (int)floorf(((float)ix - 1.f + (align ? 0.f : 0.5f)) * isw - (align ? 0.f : 0.5f)) - 1);
        ox_hi = min(Wr - 1, (int)ceilf(((float)ix + 1.f + (align ? 0.f : 0.5f)) * isw - (align ? 0.f : 0.5f)) + 1);
      }
      for (int oy = oy_lo + rs; oy <= oy_hi; oy += RS) {
        int y0, y1;
        float ly0, ly1;
        src_index(oy, sh, Hi, align, y0, y1, ly0, ly1);
        const float wy = (y0 == iy ? ly0 : 0.f) + (y1 == iy ? ly1 : 0.f);
        if (wy == 0.f) continue;
        const float* row = dout + (((size_t)b * Hout + oy + py) * Wout + px) * lddout + 4 * cq;
        for (int ox = ox_lo; ox <= ox_hi; ++ox) {
          int x0, x1;
          float lx0, lx1;
          src_index(ox, sw, Wi, align, x0, x1, lx0, lx1);
          const float wx = (x0 == ix ? lx0 : 0.f) + (x1 == ix ? lx1 : 0.f);
          if (wx == 0.f) continue;
          s += (wy * wx) * ld4(row + (size_t)ox * lddout);
        }
      }
    }
    if (RS > 1) {
      __syncthreads();
      red[threadIdx.x] = s;
      __syncthreads();
      if (active && rs == 0) {
#pragma unroll
        for (int r = 1; r < RS; ++r) s += red[threadIdx.x + r * Q * P2];
      }
    }
    if (active && rs == 0 && pix < npix) {
      float* d = din + pix * lddin + 4 * cq;
      st4(d, acc ? ld4(d) + s : s);
    }
  }
}

// The same transpose onto up to three targets in ONE launch (hrseg_bilinear_bwd_multi: the backward of head_mix_kernel and of
// the HRNet fuse layers, all C channels of dout onto every target).  Two bodies; hrseg_bilinear_bwd_multi holds the rule.
// absmax (optional, [n][64], zeroed by the caller): max|din| per target as hrseg_absmax leaves it (an integer maximum:
// order-independent).
//
// GATHER body (bilinear_bwd_multi_kernel): bilinear_bwd_kernel's weights, (wy * wx) * g products and row order.  Threads =
// `qs` channel quads (one of C / 4 / qs channel slabs) x `lanes`; a block works on one target: rs[t] lanes split the footprint
// rows of a pixel and are added in lane order through LDS, lanes / rs[t] pixels per block.  Every element of dout is loaded
// four times per target, and no block order makes the re-reads hit L2 (profiles/README.md "Shared head at branch resolution":
// they are served by the Infinity Cache at about 8 TB/s).  Kept for the shapes the streaming body refuses.
//
// STREAMING body (bilinear_bwd_stream_kernel, below it): dout comes from global memory about once and the reuse happens on
// chip.  A block owns (channel slab, image, band); a band is the same range of target rows per target as in the gather body.
// The block streams the rows of dout that carry weight for its target rows, in ascending oy, through a two-slot ring in LDS
// (row oy + 1 is in flight in registers while row oy is consumed); neighbouring bands re-read the halo rows.  A thread owns up
// to BWD_STREAM_ITEMS fixed items (target, ix, channel quad) and keeps two live target rows of each in registers:
//   column pass  c = sum_k wx[k] * g[xa + k], ascending k, from the LDS row (xa, count and wx[] tabulated once per block,
//                zero weights at the edges trimmed, as in the gather body);
//   row pass     acc[y0] += w0 * c, acc[y0 + 1] += w1 * c (y0, w0, w1 tabulated per (target, oy) once per block; a weight
//                of exactly 0 is never multiplied: a NaN of dout stays inside its 2 x 2 support);
//   a target row is stored (and folded into absmax) once oy has passed its last contributing row.
// The sum of a target element is wy * (sum wx * g) over ascending oy whatever the band count, the slab width and the grid:
// the output bits do not depend on either knob.  No float atomics.
struct BilinearBwdMultiArgs {
  const float* dout; int lddout;
  int B, Hout, Wout, C, n, align, lanes, nbands, qs;
  float* din[3]; int lddin[3]; int Hi[3], Wi[3];
  float sh[3], sw[3];
  int rs[3];             // row splits per pixel (power of two, divides lanes)
  int nx[3], ny[3];      // most columns / rows of a footprint (table sizes)
  int blk_end[3];        // blocks per (image, band): running sum over the targets
  float* absmax;
};
__global__ __launch_bounds__(1024) void bilinear_bwd_multi_kernel(BilinearBwdMultiArgs a) {
  __shared__ f32x4 red[1024];
  __shared__ int meta[16][4];            // per pixel lane: first live row, rows, first live column, columns
  extern __shared__ float wtab[];        // per pixel lane: wx[nx[t]], wy[ny[t]]
  const int Q = a.qs;
  const int ln = threadIdx.x / Q;
  const bool active = ln < a.lanes;
  const int per = a.blk_end[a.n - 1];
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int bk = bid / per;
  int r = bid - bk * per;
  const int slab = bk / (a.B * a.nbands), ib = bk - slab * (a.B * a.nbands);
  const int b = ib / a.nbands, band = ib - b * a.nbands;
  const int cq = slab * Q + threadIdx.x % Q;
  int t = 0;
  while (t + 1 < a.n && r >= a.blk_end[t]) ++t;
  if (t) r -= a.blk_end[t - 1];
  const int Hi = a.Hi[t], Wi = a.Wi[t], RS = a.rs[t], PL = a.lanes / RS;
  const float sh = a.sh[t], sw = a.sw[t];
  const int Hr = a.Hout, Wr = a.Wout, align = a.align;
  const int pl = ln % PL, rsi = ln / PL;
  // target rows of this band: [ceil(band * Hi / nbands), ceil((band + 1) * Hi / nbands))
  const int r0 = (band * Hi + a.nbands - 1) / a.nbands, r1 = ((band + 1) * Hi + a.nbands - 1) / a.nbands;
  const int q = r * PL + pl;
  const bool valid = active && q < (r1 - r0) * Wi;
  const int iy = r0 + q / Wi, ix = q % Wi;
  const float ish = sh > 0.f ? 1.f / sh : 0.f, isw = sw > 0.f ? 1.f / sw : 0.f;
  // The weights of a pixel's footprint depend on the pixel alone, not on the channel or (wx) the row: the first thread of a
  // pixel lane tabulates them in LDS once -- first live column and row, their counts, wx[] and wy[] with the zero weights at
  // the edges trimmed (bilinear_bwd_kernel skips those terms) -- instead of every thread evaluating src_index for every
  // (row, column) it visits, which is what bounded this kernel (instruction issue, not memory)
  float* wxt = wtab + pl * (a.nx[t] + a.ny[t]);
  float* wyt = wxt + a.nx[t];
  if (valid && rsi == 0 && threadIdx.x % Q == 0) {
    int oy_lo = 0, oy_hi = Hr - 1, ox_lo = 0, ox_hi = Wr - 1;
    if (sh > 0.f) {
      oy_lo = max(0, (int)floorf(((float)iy - 1.f + (align ? 0.f : 0.5f)) * ish - (align ? 0.f : 0.5f)) - 1);
      oy_hi = min(Hr - 1, (int)ceilf(((float)iy + 1.f + (align ? 0.f : 0.5f)) * ish - (align ? 0.f : 0.5f)) + 1);
    }
    if (sw > 0.f) {
      ox_lo = max(0, (int)floorf(((float)ix - 1.f + (align ? 0.f : 0.5f)) * isw - (align ? 0.f : 0.5f)) - 1);
      ox_hi = min(Wr - 1, (int)ceilf(((float)ix + 1.f + (align ? 0.f : 0.5f)) * isw - (align ? 0.f : 0.5f)) + 1);
    }
    int ya = -1, ny = 0, xa = -1, nx = 0;
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
      int y0, y1;
      float ly0, ly1;
      src_index(oy, sh, Hi, align, y0, y1, ly0, ly1);
      const float wy = (y0 == iy ? ly0 : 0.f) + (y1 == iy ? ly1 : 0.f);
      if (ya < 0 && wy != 0.f) ya = oy;
      if (ya >= 0 && oy - ya < a.ny[t]) {
        wyt[oy - ya] = wy;
        if (wy != 0.f) ny = oy - ya + 1;
      }
    }
    for (int ox = ox_lo; ox <= ox_hi; ++ox) {
      int x0, x1;
      float lx0, lx1;
      src_index(ox, sw, Wi, align, x0, x1, lx0, lx1);
      const float wx = (x0 == ix ? lx0 : 0.f) + (x1 == ix ? lx1 : 0.f);
      if (xa < 0 && wx != 0.f) xa = ox;
      if (xa >= 0 && ox - xa < a.nx[t]) {
        wxt[ox - xa] = wx;
        if (wx != 0.f) nx = ox - xa + 1;
      }
    }
    meta[pl][0] = ya; meta[pl][1] = ny; meta[pl][2] = xa; meta[pl][3] = nx;
  }
  __syncthreads();
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (valid) {
    const int ya = meta[pl][0], ny = meta[pl][1], xa = meta[pl][2], nx = meta[pl][3];
    for (int i = rsi; i < ny; i += RS) {
      const float wy = wyt[i];
      if (wy == 0.f) continue;
      const float* row = a.dout + (((size_t)b * Hr + ya + i) * Wr + xa) * a.lddout + 4 * cq;
#pragma unroll 4
      for (int k = 0; k < nx; ++k) s += (wy * wxt[k]) * ld4(row + (size_t)k * a.lddout);
    }
  }
  if (RS > 1) {                            // (one target per block: the branch is uniform)
    red[threadIdx.x] = s;
    __syncthreads();
    if (valid && rsi == 0) {
      for (int k = 1; k < RS; ++k) s += red[threadIdx.x + k * Q * PL];
    }
  }
  float amax = 0.f;
  if (valid && rsi == 0) {
    st4(a.din[t] + (((size_t)b * Hi + iy) * Wi + ix) * a.lddin[t] + 4 * cq, s);
#pragma unroll
    for (int j = 0; j < 4; ++j) amax = fmaxf(amax, abs_nan_inf(s[j]));
  }
  if (a.absmax) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    if ((threadIdx.x & 63) == 0 && amax > 0.f)
      atomicMax(reinterpret_cast<unsigned*>(a.absmax) + t * 64 + (bid & 63), __float_as_uint(amax));
  }
}

#define BWD_STREAM_ITEMS 4       // (target, ix, channel quad) items and 16-byte row loads per thread, at most
struct BilinearBwdStreamArgs {
  const float* dout; int lddout;
  int B, H, W, C, n, align, nbands, SQ;      // SQ: channel quads of a slab (the last slab may hold fewer)
  float* din[3]; int lddin[3]; int Hi[3], Wi[3];
  float sh[3], sw[3];
  int nx[3];             // most columns of a footprint (row length of the target's wx table)
  int col0[4];           // running sum of Wi: first entry of the target in the column tables
  int wx0[3];            // first float of the target's wx table
  float* absmax;
};
// dynamic LDS: ring [2][W * SQ] f32x4 | row table y0 [n * H] int, w0 [n * H], w1 [n * H] | column table (xa, count) [col0[n]]
// | wx tables
__global__ __launch_bounds__(1024) void bilinear_bwd_stream_kernel(BilinearBwdStreamArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int range[2];                 // first and last row of dout with weight on the band
  __shared__ unsigned bmax[3];
  __shared__ int band_r0[3], band_r1[3];
  constexpr int NI = BWD_STREAM_ITEMS;
  const int T = blockDim.x, tid = threadIdx.x;
  const int H = a.H, W = a.W, n = a.n, ncol = a.col0[n];
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  // the slabs of one (image, band) follow each other on one XCD (xcd_remap) and stream the same rows at about the same time:
  // a slab's pieces of a pixel (192 bytes at a 2880-byte stride) share their first and last 128-byte line with the
  // neighbouring slabs, and whichever block comes second finds the line in L2 instead of fetching it again
  const int nslab = ((a.C >> 2) + a.SQ - 1) / a.SQ;
  const int slab = bid % nslab, ib = bid / nslab;
  const int band = ib % a.nbands, b = ib / a.nbands;
  const int q0 = slab * a.SQ, sq = min(a.SQ, (a.C >> 2) - q0);
  const int rq = W * a.SQ;                 // quads of a ring slot
  f32x4* const ring = reinterpret_cast<f32x4*>(smem);
  int* const rowy = reinterpret_cast<int*>(smem + (size_t)8 * rq);
  float* const roww0 = reinterpret_cast<float*>(rowy + n * H);
  float* const roww1 = roww0 + n * H;
  int* const colm = reinterpret_cast<int*>(roww1 + n * H);
  float* const wxtab = reinterpret_cast<float*>(colm + 2 * ncol);
  if (tid == 0) { range[0] = H; range[1] = -1; }
  if (tid < 3) {
    bmax[tid] = 0u;
    if (tid < n) {         // target rows of this band: [ceil(band * Hi / nbands), ceil((band + 1) * Hi / nbands))
      band_r0[tid] = (int)(((long)band * a.Hi[tid] + a.nbands - 1) / a.nbands);
      band_r1[tid] = (int)(((long)(band + 1) * a.Hi[tid] + a.nbands - 1) / a.nbands);
    }
  }
  __syncthreads();
  // row table: dout row oy feeds target rows y0 (weight w0) and y0 + 1 (w1); both taps on one row add up as in the gather
  // bodies, and a weight onto a row of another band is entered as 0: the row pass skips it
  for (int e = tid; e < n * H; e += T) {
    const int t = e / H, oy = e - t * H;
    int y0, y1;
    float ly0, ly1;
    src_index(oy, a.sh[t], a.Hi[t], a.align, y0, y1, ly0, ly1);
    float w0 = (y1 == y0) ? ly0 + ly1 : ly0, w1 = (y1 == y0) ? 0.f : ly1;
    if (y0 < band_r0[t] || y0 >= band_r1[t]) w0 = 0.f;
    if (y0 + 1 < band_r0[t] || y0 + 1 >= band_r1[t]) w1 = 0.f;
    rowy[e] = y0; roww0[e] = w0; roww1[e] = w1;
    if (w0 != 0.f || w1 != 0.f) {
      atomicMin(&range[0], oy);
      atomicMax(&range[1], oy);
    }
  }
  // column table: first live column, live columns and wx[] of every (target, ix), the zero weights at the edges trimmed
  for (int e = tid; e < ncol; e += T) {
    int t = 0;
    while (t + 1 < n && e >= a.col0[t + 1]) ++t;
    const int ix = e - a.col0[t], Wi = a.Wi[t], align = a.align;
    const float sw = a.sw[t], isw = sw > 0.f ? 1.f / sw : 0.f;
    int ox_lo = 0, ox_hi = W - 1;
    if (sw > 0.f) {
      ox_lo = max(0, (int)floorf(((float)ix - 1.f + (align ? 0.f : 0.5f)) * isw - (align ? 0.f : 0.5f)) - 1);
      ox_hi = min(W - 1, (int)ceilf(((float)ix + 1.f + (align ? 0.f : 0.5f)) * isw - (align ? 0.f : 0.5f)) + 1);
    }
    float* wxt = wxtab + a.wx0[t] + ix * a.nx[t];
    int xa = -1, nx = 0;
    for (int ox = ox_lo; ox <= ox_hi; ++ox) {
      int x0, x1;
      float lx0, lx1;
      src_index(ox, sw, Wi, align, x0, x1, lx0, lx1);
      const float wx = (x0 == ix ? lx0 : 0.f) + (x1 == ix ? lx1 : 0.f);
      if (xa < 0 && wx != 0.f) xa = ox;
      if (xa >= 0 && ox - xa < a.nx[t]) {
        wxt[ox - xa] = wx;
        if (wx != 0.f) nx = ox - xa + 1;
      }
    }
    colm[2 * e] = xa < 0 ? 0 : xa;
    colm[2 * e + 1] = nx;
  }
  __syncthreads();
  // this thread's items (item e = tid + i * T over (column entry, quad of the slab)) and row loads (quad j = tid + l * T of a row)
  int it_t[NI], it_nx[NI], it_g[NI], it_w[NI], it_out[NI];       // it_out: the item's element of target row 0, from din[t]
  f32x4 acc0[NI], acc1[NI];
  int ld_off[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int e = tid + i * T;
    const bool valid = e < ncol * sq;
    const int col = valid ? e / sq : 0, q = valid ? e - col * sq : 0;
    int t = 0;
    while (t + 1 < n && col >= a.col0[t + 1]) ++t;
    const int ix = col - a.col0[t];
    it_t[i] = valid ? t : -1;
    it_nx[i] = valid ? colm[2 * col + 1] : 0;
    it_g[i] = colm[2 * col] * sq + q;
    it_w[i] = a.wx0[t] + ix * a.nx[t];
    it_out[i] = (b * a.Hi[t] * a.Wi[t] + ix) * a.lddin[t] + 4 * (q0 + q);
    acc0[i] = acc1[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int j = min(tid + i * T, W * sq - 1);        // (past the row: the last quad again, no branch around the load)
    const int x = j / sq;
    ld_off[i] = x * a.lddout + 4 * (q0 + j - x * sq);
  }
  // The live target rows are the same in every thread: acc0 holds row cur[t] of the item's target, acc1 row cur[t] + 1.
  // rotate(t): row cur[t] is complete -- store it if it is the band's -- and the next row moves up.
  int cur[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) cur[t] = t < n ? __builtin_amdgcn_readfirstlane(band_r0[t]) - 1 : 0;
  auto rotate = [&](int t) {
    const bool mine = cur[t] >= band_r0[t] && cur[t] < band_r1[t];
    float* const row = a.din[t] + (long)cur[t] * a.Wi[t] * a.lddin[t];
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      if (it_t[i] != t) continue;
      if (mine) {
        st4(row + it_out[i], acc0[i]);
#pragma unroll
        for (int j = 0; j < 4; ++j) m = fmaxf(m, abs_nan_inf(acc0[i][j]));
      }
      acc0[i] = acc1[i];
      acc1[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (a.absmax && m > 0.f) atomicMax(&bmax[t], __float_as_uint(m));
    ++cur[t];
  };
  const int oy_lo = range[0], oy_hi = range[1];
  const float* const img = a.dout + (size_t)b * H * W * a.lddout;
  f32x4 v[NI];
  auto load = [&](int oy) {
    const float* row = img + (size_t)oy * W * a.lddout;
#pragma unroll
    for (int l = 0; l < NI; ++l)
      if (l * T < W * sq) v[l] = ld4(row + ld_off[l]);          // (uniform)
  };
  auto write = [&](f32x4* slot) {
#pragma unroll
    for (int l = 0; l < NI; ++l)
      if (tid + l * T < W * sq) slot[tid + l * T] = v[l];
  };
  if (oy_lo <= oy_hi) {
    load(oy_lo);
    write(ring);
    __syncthreads();
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
      // row oy + 1 is in flight while row oy is consumed; it goes into the slot that row oy - 1 was read from (every thread
      // has passed the barrier that ended that trip)
      const bool more = oy < oy_hi;
      if (more) load(oy + 1);
      const f32x4* g = ring + ((oy - oy_lo) & 1) * rq;
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        if (t >= n) continue;
        const float w0 = roww0[t * H + oy], w1 = roww1[t * H + oy];      // (the same in every thread: the branches are uniform)
        if (w0 == 0.f && w1 == 0.f) continue;
        const int y0 = __builtin_amdgcn_readfirstlane(rowy[t * H + oy]);
        while (cur[t] < y0) rotate(t);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          if (it_t[i] != t) continue;
          const f32x4* gi = g + it_g[i];
          const float* wx = wxtab + it_w[i];
          f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
          for (int k = 0; k < it_nx[i]; ++k) {
            const f32x4 gv = gi[k * sq];
            const float w = wx[k];
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j] = __builtin_fmaf(w, gv[j], c[j]);
          }
          if (w0 != 0.f) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc0[i][j] = __builtin_fmaf(w0, c[j], acc0[i][j]);
          }
          if (w1 != 0.f) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc1[i][j] = __builtin_fmaf(w1, c[j], acc1[i][j]);
          }
        }
      }
      if (more) write(ring + ((oy + 1 - oy_lo) & 1) * rq);
      __syncthreads();
    }
  }
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    if (t >= n) continue;
    while (cur[t] < band_r1[t]) rotate(t);
  }
  if (a.absmax) {
    __syncthreads();
    if (tid < n && bmax[tid] > 0u) atomicMax(reinterpret_cast<unsigned*>(a.absmax) + tid * 64 + (bid & 63), bmax[tid]);
  }
}

// --------------------------------------------------------------------------- small glue
// column blocks of a convolution weight [rows = Cout * taps][Cin] <-> n contiguous [rows][width_j] blocks laid end to end
// (hrseg_weight_cols_gather / hrseg_weight_cols_scatter_add): the operands and the gradient staging of a layer that is
// computed per input-channel block (the HRNet head at branch resolution)
struct WeightColsArgs {
  int n, rows, Cin;
  int col0[9];           // first column of block j (col0[n] = Cin), all multiples of 4
};
__global__ __launch_bounds__(256) void weight_cols_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                          WeightColsArgs a, int scatter_add) {
  const int Q = a.Cin >> 2;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)a.rows * Q) return;
  const int row = (int)(i / Q), c = 4 * (int)(i - (long)row * Q);
  int j = 0;
  while (j + 1 < a.n && c >= a.col0[j + 1]) ++j;
  const int w = a.col0[j + 1] - a.col0[j];
  const size_t full = (size_t)row * a.Cin + c, blk = (size_t)a.rows * a.col0[j] + (size_t)row * w + (c - a.col0[j]);
  if (scatter_add) st4(dst + full, ld4(dst + full) + ld4(src + blk));
  else st4(dst + blk, ld4(src + full));
}

__global__ __launch_bounds__(256) void add_kernel(const float* __restrict__ a, int lda, const float* __restrict__ b,
                                                  int ldb, float* __restrict__ out, int ldo, int relu, long npix,
                                                  int C) {
  const Lanes L = make_lanes(C);
  if (!L.active) return;
  FOR_PIXELS(pix, L, npix) {
    f32x4 v = ld4(a + pix * lda + 4 * L.cq) + ld4(b + pix * ldb + 4 * L.cq);
    if (relu) v = relu_nan(v);
    st4(out + pix * ldo + 4 * L.cq, v);
  }
}
__global__ __launch_bounds__(256) void copy_kernel(const float* __restrict__ in, int ldin, float* __restrict__ out,
                                                   int ldout, int acc, long npix, int C) {
  const Lanes L = make_lanes(C);
  if (!L.active) return;
  FOR_PIXELS(pix, L, npix) {
    f32x4 v = ld4(in + pix * ldin + 4 * L.cq);
    float* o = out + pix * ldout + 4 * L.cq;
    st4(o, acc ? ld4(o) + v : v);
  }
}
__global__ __launch_bounds__(256) void relu_bwd_kernel(const float* __restrict__ dz, int lddz,
                                                       const float* __restrict__ z, int ldz, float* __restrict__ dx,
                                                       int lddx, long npix, int C) {
  const Lanes L = make_lanes(C);
  if (!L.active) return;
  FOR_PIXELS(pix, L, npix) {
    f32x4 g = ld4(dz + pix * lddz + 4 * L.cq);
    const f32x4 zz = ld4(z + pix * ldz + 4 * L.cq);
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = zz[j] > 0.f ? g[j] : 0.f;
    st4(dx + pix * lddx + 4 * L.cq, g);
  }
}

// max|x| of an NHWC tensor into a 64-slot array (slot = block % 64, as hrseg_bn_bwd_t.dy_absmax); NaN counts as +Inf so
// that a non-finite tensor is never reported as in range.  `out` must be zeroed by the caller (hrseg_fill).
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ x, int ldx, long npix, int C,
                                                     float* __restrict__ out) {
  const Lanes L = make_lanes(C);
  float amax = 0.f;
  if (L.active) {
    FOR_PIXELS(pix, L, npix) {
      const f32x4 v = ld4(x + pix * ldx + 4 * L.cq);
#pragma unroll
      for (int j = 0; j < 4; ++j) amax = fmaxf(amax, abs_nan_inf(v[j]));
    }
  }
  __shared__ float wmax[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = amax;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    if (m > 0.f) atomicMax(reinterpret_cast<unsigned*>(out) + (blockIdx.x & 63), __float_as_uint(m));
  }
}

// NCHW <-> NHWC for narrow tensors (image: C=3, logits: C<=16): thread per pixel
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ in, float* __restrict__ out, int ldout, int B, int C,
                                    long hw) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * hw) return;
  const long b = i / hw, p = i - b * hw;
  for (int c = 0; c < C; ++c) out[i * ldout + c] = in[(b * C + c) * hw + p];
}
__global__ void nhwc_to_nchw_kernel(const float* __restrict__ in, int ldin, float* __restrict__ out, int B, int C,
                                    long hw) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * hw) return;
  const long b = i / hw, p = i - b * hw;
  for (int c = 0; c < C; ++c) out[(b * C + c) * hw + p] = in[i * ldin + c];
}

// =========================================================================== C ABI
extern "C" int hrseg_maxpool2_fwd(const float* x, int ldx, float* y, int ldy, int B, int Hi, int Wi, int C,
                                  hrseg_stream_t stream) {
  if (int e = check_c(C, "hrseg_maxpool2_fwd")) return e;
  HRSEG_CHECK_ARG(x && y && B > 0 && Hi >= 2 && Wi >= 2, "hrseg_maxpool2_fwd: bad arguments");
  if (int e = check_operand(x, ldx, C, "hrseg_maxpool2_fwd", "x")) return e;
  if (int e = check_operand(y, ldy, C, "hrseg_maxpool2_fwd", "y")) return e;
  const long npix = (long)B * (Hi / 2) * (Wi / 2);
  hipLaunchKernelGGL(maxpool2_fwd_kernel, dim3(elem_grid(npix, C)), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy,
                     B, Hi, Wi, C);
  HRSEG_LAUNCH_CHECK("maxpool2_fwd");
  return 0;
}

extern "C" int hrseg_maxpool2_bwd(const float* x, int ldx, const float* dy, int lddy, float* dx, int lddx,
                                  int accumulate, int B, int Hi, int Wi, int C, hrseg_stream_t stream) {
  if (int e = check_c(C, "hrseg_maxpool2_bwd")) return e;
  HRSEG_CHECK_ARG(x && dy && dx && B > 0 && Hi >= 2 && Wi >= 2, "hrseg_maxpool2_bwd: bad arguments");
  if (int e = check_operand(x, ldx, C, "hrseg_maxpool2_bwd", "x")) return e;
  if (int e = check_operand(dy, lddy, C, "hrseg_maxpool2_bwd", "dy")) return e;
  if (int e = check_operand(dx, lddx, C, "hrseg_maxpool2_bwd", "dx")) return e;
  const long ncell = (long)B * ((Hi + 1) / 2) * ((Wi + 1) / 2);
  hipLaunchKernelGGL(maxpool2_bwd_kernel, dim3(elem_grid(ncell, C)), dim3(256), 0, (hipStream_t)stream, x, ldx, dy,
                     lddy, dx, lddx, accumulate, B, Hi, Wi, C);
  HRSEG_LAUNCH_CHECK("maxpool2_bwd");
  return 0;
}

extern "C" int hrseg_bilinear_fwd(const float* in, int ldin, int B, int Hi, int Wi, int C, float* out, int ldout,
                                  int Hout, int Wout, int Hr, int Wr, int py, int px, int align_corners,
                                  int accumulate, int relu, hrseg_stream_t stream) {
  if (int e = check_c(C, "hrseg_bilinear_fwd")) return e;
  HRSEG_CHECK_ARG(in && out && B > 0 && Hi > 0 && Wi > 0 && Hr > 0 && Wr > 0 && py >= 0 && px >= 0 &&
                      py + Hr <= Hout && px + Wr <= Wout,
                  "hrseg_bilinear_fwd: placed image %dx%d at (%d,%d) does not fit %dx%d", Hr, Wr, py, px, Hout, Wout);
  if (int e = check_operand(in, ldin, C, "hrseg_bilinear_fwd", "in")) return e;
  if (int e = check_operand(out, ldout, C, "hrseg_bilinear_fwd", "out")) return e;
  const long npix = (long)B * Hout * Wout;
  hipLaunchKernelGGL(bilinear_fwd_kernel, dim3(elem_grid(npix, C)), dim3(256), 0, (hipStream_t)stream, in, ldin, B, Hi,
                     Wi, C, out, ldout, Hout, Wout, Hr, Wr, py, px, resize_scale(Hi, Hr, align_corners),
                     resize_scale(Wi, Wr, align_corners), align_corners, accumulate, relu);
  HRSEG_LAUNCH_CHECK("bilinear_fwd");
  return 0;
}

extern "C" int hrseg_bilinear_bwd(const float* dout, int lddout, int B, int Hi, int Wi, int C, float* din, int lddin,
                                  int Hout, int Wout, int Hr, int Wr, int py, int px, int align_corners,
                                  int accumulate, hrseg_stream_t stream) {
  if (int e = check_c(C, "hrseg_bilinear_bwd")) return e;
  HRSEG_CHECK_ARG(dout && din && B > 0 && Hi > 0 && Wi > 0 && Hr > 0 && Wr > 0 && py >= 0 && px >= 0 &&
                      py + Hr <= Hout && px + Wr <= Wout,
                  "hrseg_bilinear_bwd: bad geometry");
  if (int e = check_operand(dout, lddout, C, "hrseg_bilinear_bwd", "dout")) return e;
  if (int e = check_operand(din, lddin, C, "hrseg_bilinear_bwd", "din")) return e;
  const long npix = (long)B * Hi * Wi;
  // row splits: enough blocks to fill the chip, at most half the footprint rows, Q*RS <= 256
  const int Q = C / 4;
  const int foot = (Hi > 1 && Hr > 1) ? (int)(2.0 * (Hr - 1) / (Hi - 1)) + 3 : Hr;
  int rs = 1;
  while (rs < 8 && Q * rs * 2 <= 256 && rs * 2 <= foot / 2 && npix / max(1, 256 / (Q * rs)) < 1024) rs *= 2;
  const int P2 = max(1, 256 / (Q * rs));
  long blocks = (npix + P2 - 1) / P2;
  if (blocks > 4096) blocks = 4096;
  const float sh = resize_scale(Hi, Hr, align_corners), sw = resize_scale(Wi, Wr, align_corners);
#define HRSEG_BIL(RS_) hipLaunchKernelGGL(bilinear_bwd_kernel<RS_>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, \
                                          dout, lddout, B, Hi, Wi, C, din, lddin, Hout, Wout, Hr, Wr, py, px, sh, sw,         \
                                          align_corners, accumulate)
  if (rs == 1) HRSEG_BIL(1); else if (rs == 2) HRSEG_BIL(2); else if (rs == 4) HRSEG_BIL(4); else HRSEG_BIL(8);
#undef HRSEG_BIL
  HRSEG_LAUNCH_CHECK("bilinear_bwd");
  return 0;
}

extern "C" int hrseg_fuse_sum(int n_same, const float* const* same, const int* ld_same, int n_low, const float* const* low,
                              const int* ld_low, const int* Hi, const int* Wi, float* out, int ldo, int B, int H, int W, int C,
                              int align_corners, int relu, hrseg_stream_t stream) {
  if (int e = check_c(C, "hrseg_fuse_sum")) return e;
  HRSEG_CHECK_ARG(n_same >= 1 && n_same <= 4 && n_low >= 0 && n_low <= 3 && same && ld_same && out && B > 0 && H > 0 && W > 0,
                  "hrseg_fuse_sum: 1..4 same-resolution terms and 0..3 low-resolution terms");
  HRSEG_CHECK_ARG(n_low == 0 || (low && ld_low && Hi && Wi), "hrseg_fuse_sum: low-resolution terms need their geometry");
  if (int e = check_operand(out, ldo, C, "hrseg_fuse_sum", "out")) return e;
  FuseSumArgs a{};
  a.n_same = n_same; a.n_low = n_low;
  for (int i = 0; i < n_same; ++i) {
    HRSEG_CHECK_ARG(same[i] && ld_same[i] >= C && ld_same[i] % 4 == 0 && al16(same[i]), "hrseg_fuse_sum: bad same-resolution term %d", i);
    a.same[i] = same[i]; a.ld_same[i] = ld_same[i];
  }
  for (int j = 0; j < n_low; ++j) {
    HRSEG_CHECK_ARG(low[j] && ld_low[j] >= C && ld_low[j] % 4 == 0 && al16(low[j]) && Hi[j] > 0 && Wi[j] > 0, "hrseg_fuse_sum: bad low-resolution term %d", j);
    a.low[j] = low[j]; a.ld_low[j] = ld_low[j]; a.Hi[j] = Hi[j]; a.Wi[j] = Wi[j];
    a.sh[j] = resize_scale(Hi[j], H, align_corners);
    a.sw[j] = resize_scale(Wi[j], W, align_corners);
  }
  a.out = out; a.ldo = ldo; a.B = B; a.H = H; a.W = W; a.C = C; a.align = align_corners; a.relu = relu;
  const long npix = (long)B * H * W;
  hipLaunchKernelGGL(fuse_sum_kernel, dim3(elem_grid(npix, C)), dim3(256), 0, (hipStream_t)stream, a);
  HRSEG_LAUNCH_CHECK("fuse_sum");
  return 0;
}

extern "C" int hrseg_head_mix(float* y, int ldy, const float* bias, int n_low, const float* const* low, const int* ld_low,
                              const int* Hi, const int* Wi, int B, int H, int W, int C, int align_corners, double* partial,
                              int nchunks, hrseg_stream_t stream) {
  if (int e = check_c(C, "hrseg_head_mix")) return e;
  HRSEG_CHECK_ARG(y && ldy >= C && ldy % 4 == 0 && n_low >= 0 && n_low <= 3 && B > 0 && H > 0 && W > 0,
                  "hrseg_head_mix: bad arguments (0..3 low-resolution terms, ldy=%d C=%d)", ldy, C);
  HRSEG_CHECK_ARG(n_low == 0 || (low && ld_low && Hi && Wi), "hrseg_head_mix: low-resolution terms need their geometry");
  const long npix = (long)B * H * W;
  HRSEG_CHECK_ARG(nchunks >= 1 && nchunks <= npix && nchunks <= 65535, "hrseg_head_mix: nchunks=%d must be in [1, min(pixels, 65535)]", nchunks);
  HeadMixArgs a{};
  a.y = y; a.ldy = ldy; a.bias = bias; a.n_low = n_low;
  for (int j = 0; j < n_low; ++j) {
    HRSEG_CHECK_ARG(low[j] && ld_low[j] >= C && ld_low[j] % 4 == 0 && Hi[j] > 0 && Wi[j] > 0, "hrseg_head_mix: bad low-resolution term %d", j);
    a.low[j] = low[j]; a.ld_low[j] = ld_low[j]; a.Hi[j] = Hi[j]; a.Wi[j] = Wi[j];
    a.sh[j] = resize_scale(Hi[j], H, align_corners);
    a.sw[j] = resize_scale(Wi[j], W, align_corners);
  }
  a.B = B; a.H = H; a.W = W; a.C = C; a.align = align_corners; a.partial = partial; a.nchunks = nchunks;
  a.lanes = head_mix_lanes(C);
  hipLaunchKernelGGL(head_mix_kernel, dim3(nchunks), dim3((C / 4 * a.lanes + 63) / 64 * 64), 0, (hipStream_t)stream, a);
  HRSEG_LAUNCH_CHECK("head_mix");
  return 0;
}

// The streaming body's plan.  -> 1 launched, 0 the shape is not its own (the caller runs the gather body), < 0 an error.
//  * slab: the widest one whose row of dout (W x slab quads) and whose items (sum of Wi x slab quads) are at most
//    BWD_STREAM_ITEMS per thread of a 512-thread block and whose ring is at most 64 KiB (two blocks per CU beside the tables):
//    12 quads = 192 contiguous bytes per pixel at 155 columns, 15 slabs of the head's 720 channels.  A divisor of C / 4 where
//    one lies in the upper half of that range, else a ragged last slab.  hrseg_tune bwd_multi_slab (channels) overrides it; a
//    forced slab may take 1024 threads and one block per CU.
//  * bands: as many as keep every block resident at once (BWD_STREAM_BLOCKS = two per CU; a fifth band at the head's shape
//    starts a second round of blocks: 270 us with four, 352 with five), at most the rows of the coarsest target.
//    hrseg_tune bwd_multi_bands overrides, clamped likewise.
//  * the rule between the bodies, measured in isolation on MI355X (profiles/README.md "Streaming bilinear transpose"): a block
//    streams its rows one after the other, so the body needs (slab, image) pairs -- at least a block per CU with
//    BWD_STREAM_BANDS bands.  Head, 720 ch x 155 x 155 x 8 images, 120 pairs: streaming 270 us, gather 448 us.  Fuse layers,
//    one slab x 8 images: streaming 69 / 28 / 11.5 us at its best band count (48 ch x 155 onto three targets / 96 x 78 onto
//    two / 192 x 39 onto one), gather 36 / 16 / 10.3 us -- their gradients (12-49 MB) stay in the Infinity Cache and the
//    re-reads cost little: they keep the gather body.  A knob that is set sends the shape to the streaming body regardless.
#define BWD_STREAM_BLOCKS 512
#define BWD_STREAM_BANDS 4
static int bilinear_bwd_stream(BilinearBwdStreamArgs& a, hipStream_t stream) {
  const int Q = a.C / 4, W = a.W, n = a.n;
  int cols = 0, wx = 0, hmin = a.Hi[0];
  for (int j = 0; j < n; ++j) {
    a.col0[j] = cols; a.wx0[j] = wx;
    cols += a.Wi[j];
    wx += a.Wi[j] * a.nx[j];
    if (a.Hi[j] < hmin) hmin = a.Hi[j];
    if ((long)a.B * a.Hi[j] * a.Wi[j] * a.lddin[j] >= 2147483647L) return 0;      // (the kernel's element offsets are ints)
    // a target larger than dout (no model issues one) has footprints of one or two terms: against hrseg_bilinear_bwd the
    // separable products' extra rounding is not covered by 2 * n * 2^-24 * A at n = 1
    if (a.Hi[j] > a.H || a.Wi[j] > W) return 0;
  }
  a.col0[n] = cols;
  const int wide = cols > W ? cols : W;                          // quads of work per slab quad: loads or items, the larger
  if ((long)W * a.lddout >= 2147483647L) return 0;
  const size_t tables = ((size_t)3 * n * a.H + 2 * cols + wx) * sizeof(float);
  auto ring_bytes = [&](int sq) { return (size_t)2 * W * sq * 16; };
  int sq = hrseg_g_bwd_multi_slab / 4;
  if (sq > 0) {                                                  // forced: clamped to what one block can hold
    if (sq > Q) sq = Q;
    while (sq > 1 && ((long)wide * sq > BWD_STREAM_ITEMS * 1024 || ring_bytes(sq) + tables > 150 * 1024)) --sq;
  } else {
    int most = Q;
    while (most > 1 && ((long)wide * most > BWD_STREAM_ITEMS * 512 || ring_bytes(most) > 64 * 1024)) --most;
    sq = most;
    for (int d = most; 2 * d > most; --d)
      if (Q % d == 0) { sq = d; break; }
  }
  if ((long)wide * sq > BWD_STREAM_ITEMS * 1024 || ring_bytes(sq) + tables > 150 * 1024) return 0;
  const int threads = (long)wide * sq <= BWD_STREAM_ITEMS * 256 ? 256 : (long)wide * sq <= BWD_STREAM_ITEMS * 512 ? 512 : 1024;
  const int nslab = ceil_div(Q, sq);
  const bool forced = hrseg_g_bwd_multi_bands > 0 || hrseg_g_bwd_multi_slab > 0;
  if (!forced && (long)nslab * a.B * BWD_STREAM_BANDS < BWD_STREAM_BLOCKS / 2) return 0;
  int nbands = hrseg_g_bwd_multi_bands > 0 ? hrseg_g_bwd_multi_bands : (int)(BWD_STREAM_BLOCKS / ((long)nslab * a.B));
  if (nbands > hmin) nbands = hmin;
  if (nbands < 1) nbands = 1;
  a.SQ = sq; a.nbands = nbands;
  const long blocks = (long)nslab * a.B * nbands;
  HRSEG_CHECK_ARG(blocks < 2147483647L, "hrseg_bilinear_bwd_multi: %ld blocks exceed the grid", blocks);
  const size_t lds = ring_bytes(sq) + tables;
  static bool big_lds = false;
  if (lds > 48 * 1024 && !big_lds) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&bilinear_bwd_stream_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    if (e != hipSuccess) {
      hrseg_set_error("hrseg_bilinear_bwd_multi: %d bytes of LDS refused: %s", 150 * 1024, hipGetErrorString(e));
      return HRSEG_ERR_LAUNCH;
    }
    big_lds = true;
  }
  hipLaunchKernelGGL(bilinear_bwd_stream_kernel, dim3((unsigned)blocks), dim3(threads), lds, stream, a);
  HRSEG_LAUNCH_CHECK("bilinear_bwd_multi");
  return 1;
}

// Routing (the rule and its numbers: bilinear_bwd_stream above): the streaming body where there are enough (slab, image)
// pairs to fill the chip and the plan fits one block; the gather body otherwise -- small gradients, targets larger than
// dout, rows or tables too large for LDS -- and on request (hrseg_tune bwd_multi_slab < 0: tools/bwd_multi_bench.py).
extern "C" int hrseg_bilinear_bwd_multi(const float* dout, int lddout, int B, int Hout, int Wout, int C, int n,
                                        float* const* din, const int* lddin, const int* Hi, const int* Wi, int align_corners,
                                        float* absmax, hrseg_stream_t stream) {
  if (int e = check_c(C, "hrseg_bilinear_bwd_multi")) return e;
  HRSEG_CHECK_ARG(dout && lddout >= C && lddout % 4 == 0 && B > 0 && Hout > 0 && Wout > 0 && n >= 1 && n <= 3 && din && lddin &&
                      Hi && Wi,
                  "hrseg_bilinear_bwd_multi: bad arguments (1..3 targets, lddout=%d C=%d)", lddout, C);
  for (int j = 0; j < n; ++j)
    HRSEG_CHECK_ARG(din[j] && lddin[j] >= C && lddin[j] % 4 == 0 && Hi[j] > 0 && Wi[j] > 0, "hrseg_bilinear_bwd_multi: bad target %d", j);
  if (hrseg_g_bwd_multi_slab >= 0) {
    BilinearBwdStreamArgs s{};
    s.dout = dout; s.lddout = lddout; s.B = B; s.H = Hout; s.W = Wout; s.C = C; s.n = n; s.align = align_corners;
    s.absmax = absmax;
    for (int j = 0; j < n; ++j) {
      s.din[j] = din[j]; s.lddin[j] = lddin[j]; s.Hi[j] = Hi[j]; s.Wi[j] = Wi[j];
      s.sh[j] = resize_scale(Hi[j], Hout, align_corners);
      s.sw[j] = resize_scale(Wi[j], Wout, align_corners);
      s.nx[j] = s.sw[j] > 0.f ? min(Wout, (int)(2.0 / s.sw[j]) + 6) : Wout;       // (as for the gather body, below)
    }
    if (int r = bilinear_bwd_stream(s, (hipStream_t)stream)) return r < 0 ? r : 0;
  }
  BilinearBwdMultiArgs a{};
  a.dout = dout; a.lddout = lddout; a.B = B; a.Hout = Hout; a.Wout = Wout; a.C = C; a.n = n; a.align = align_corners;
  a.absmax = absmax;
  // channel slabs of at most 32 quads (the largest such divisor of C / 4: 6 x 30 at 720 channels, 480 contiguous bytes per
  // pixel); threads = quads of a slab x lanes (a power of two, at most 16, at most about 768 threads: 30 quads x 16)
  int Q = C / 4;
  const int nslab = [&] { int k = 1; while (Q % k || Q / k > 32) ++k; return k; }();
  Q /= nslab;
  a.qs = Q;
  int lanes = 1;
  while (lanes < 16 && Q * lanes * 2 <= 768) lanes *= 2;
  a.lanes = lanes;
  int nbands = Hi[0];
  for (int j = 0; j < n; ++j)
    if (Hi[j] < nbands) nbands = Hi[j];
  a.nbands = nbands;
  int end = 0, tab = 0;
  for (int j = 0; j < n; ++j) {
    a.din[j] = din[j]; a.lddin[j] = lddin[j]; a.Hi[j] = Hi[j]; a.Wi[j] = Wi[j];
    a.sh[j] = resize_scale(Hi[j], Hout, align_corners);
    a.sw[j] = resize_scale(Wi[j], Wout, align_corners);
    // row splits: a quarter of the footprint rows, at most the lanes (an 8x resize has ~18 x 18 footprints and few pixels)
    const int foot = (Hi[j] > 1 && Hout > 1) ? (int)(2.0 * (Hout - 1) / (Hi[j] - 1)) + 3 : Hout;
    int rs = 1;
    while (rs * 2 <= lanes && rs * 2 <= foot / 4) rs *= 2;
    a.rs[j] = rs;
    // a footprint spans the outputs whose source lies within one input pixel of the target: 2 / scale of them + the rounding
    // of both ends (the kernel's candidate range); scale 0: one input row / column feeds every output
    a.nx[j] = a.sw[j] > 0.f ? min(Wout, (int)(2.0 / a.sw[j]) + 6) : Wout;
    a.ny[j] = a.sh[j] > 0.f ? min(Hout, (int)(2.0 / a.sh[j]) + 6) : Hout;
    if (a.nx[j] + a.ny[j] > tab) tab = a.nx[j] + a.ny[j];
    const int rows = ceil_div(Hi[j], nbands);              // most target rows in a band
    end += ceil_div((long)rows * Wi[j], lanes / rs);
    a.blk_end[j] = end;
  }
  const long blocks = (long)nslab * B * nbands * end;
  HRSEG_CHECK_ARG(blocks < 2147483647L, "hrseg_bilinear_bwd_multi: %ld blocks exceed the grid", blocks);
  const size_t lds = (size_t)lanes * tab * sizeof(float);
  HRSEG_CHECK_ARG(lds <= 32768, "hrseg_bilinear_bwd_multi: footprints of %d weights per pixel exceed the weight table", tab);
  hipLaunchKernelGGL(bilinear_bwd_multi_kernel, dim3((unsigned)blocks), dim3((Q * lanes + 63) / 64 * 64), lds, (hipStream_t)stream, a);
  HRSEG_LAUNCH_CHECK("bilinear_bwd_multi");
  return 0;
}

static int weight_cols(const char* who, const float* src, float* dst, int rows, int Cin, int n, const int* widths, int scatter_add,
                       hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(src && dst && rows > 0 && Cin > 0 && Cin % 4 == 0 && n >= 1 && n <= 8 && widths && al16(src) && al16(dst),
                  "%s: bad arguments (1..8 column blocks, 16-byte aligned buffers, Cin=%d)", who, Cin);
  WeightColsArgs a{};
  a.n = n; a.rows = rows; a.Cin = Cin;
  int c = 0;
  for (int j = 0; j < n; ++j) {
    HRSEG_CHECK_ARG(widths[j] > 0 && widths[j] % 4 == 0, "%s: block width %d must be a positive multiple of 4", who, widths[j]);
    a.col0[j] = c;
    c += widths[j];
  }
  HRSEG_CHECK_ARG(c == Cin, "%s: block widths sum to %d, the weight has %d input channels", who, c, Cin);
  a.col0[n] = Cin;
  const long n4 = (long)rows * (Cin / 4);
  hipLaunchKernelGGL(weight_cols_kernel, dim3(ceil_div(n4, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, a, scatter_add);
  HRSEG_LAUNCH_CHECK(who);
  return 0;
}
extern "C" int hrseg_weight_cols_gather(const float* w, int rows, int Cin, int n, const int* widths, float* blocks,
                                        hrseg_stream_t stream) {
  return weight_cols("hrseg_weight_cols_gather", w, blocks, rows, Cin, n, widths, 0, stream);
}
extern "C" int hrseg_weight_cols_scatter_add(const float* blocks, int rows, int Cin, int n, const int* widths, float* dw,
                                             hrseg_stream_t stream) {
  return weight_cols("hrseg_weight_cols_scatter_add", blocks, dw, rows, Cin, n, widths, 1, stream);
}

extern "C" int hrseg_add(const float* a, int lda, const float* b, int ldb, float* out, int ldo, int relu, long npix,
                         int C, hrseg_stream_t stream) {
  if (int e = check_c(C, "hrseg_add")) return e;
  HRSEG_CHECK_ARG(a && b && out && npix > 0, "hrseg_add: bad arguments");
  if (int e = check_operand(a, lda, C, "hrseg_add", "a")) return e;
  if (int e = check_operand(b, ldb, C, "hrseg_add", "b")) return e;
  if (int e = check_operand(out, ldo, C, "hrseg_add", "out")) return e;
  hipLaunchKernelGGL(add_kernel, dim3(elem_grid(npix, C)), dim3(256), 0, (hipStream_t)stream, a, lda, b, ldb, out, ldo,
                     relu, npix, C);
  HRSEG_LAUNCH_CHECK("add");
  return 0;
}

extern "C" int hrseg_copy(const float* in, int ldin, float* out, int ldout, int accumulate, long npix, int C,
                          hrseg_stream_t stream) {
  if (int e = check_c(C, "hrseg_copy")) return e;
  HRSEG_CHECK_ARG(in && out && npix > 0, "hrseg_copy: bad arguments");
  if (int e = check_operand(in, ldin, C, "hrseg_copy", "in")) return e;
  if (int e = check_operand(out, ldout, C, "hrseg_copy", "out")) return e;
  hipLaunchKernelGGL(copy_kernel, dim3(elem_grid(npix, C)), dim3(256), 0, (hipStream_t)stream, in, ldin, out, ldout,
                     accumulate, npix, C);
  HRSEG_LAUNCH_CHECK("copy");
  return 0;
}

extern "C" int hrseg_relu_bwd(const float* dz, int lddz, const float* z, int ldz, float* dx, int lddx, long npix,
                              int C, hrseg_stream_t stream) {
  if (int e = check_c(C, "hrseg_relu_bwd")) return e;
  HRSEG_CHECK_ARG(dz && z && dx && npix > 0, "hrseg_relu_bwd: bad arguments");
  if (int e = check_operand(dz, lddz, C, "hrseg_relu_bwd", "dz")) return e;
  if (int e = check_operand(z, ldz, C, "hrseg_relu_bwd", "z")) return e;
  if (int e = check_operand(dx, lddx, C, "hrseg_relu_bwd", "dx")) return e;
  hipLaunchKernelGGL(relu_bwd_kernel, dim3(elem_grid(npix, C)), dim3(256), 0, (hipStream_t)stream, dz, lddz, z, ldz,
                     dx, lddx, npix, C);
  HRSEG_LAUNCH_CHECK("relu_bwd");
  return 0;
}

extern "C" int hrseg_absmax(const float* x, int ldx, long npix, int C, float* out64, hrseg_stream_t stream) {
  if (int e = check_c(C, "hrseg_absmax")) return e;
  HRSEG_CHECK_ARG(x && out64 && npix > 0, "hrseg_absmax: bad arguments");
  if (int e = check_operand(x, ldx, C, "hrseg_absmax", "x")) return e;
  hipLaunchKernelGGL(absmax_kernel, dim3(elem_grid(npix, C)), dim3(256), 0, (hipStream_t)stream, x, ldx, npix, C, out64);
  HRSEG_LAUNCH_CHECK("absmax");
  return 0;
}

extern "C" int hrseg_nchw_to_nhwc(const float* in, float* out, int ldout, int B, int C, int H, int W,
                                  hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(in && out && B > 0 && C > 0 && H > 0 && W > 0 && ldout >= C, "hrseg_nchw_to_nhwc: bad arguments");
  const long n = (long)B * H * W;
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, in, out, ldout, B,
                     C, (long)H * W);
  HRSEG_LAUNCH_CHECK("nchw_to_nhwc");
  return 0;
}

extern "C" int hrseg_nhwc_to_nchw(const float* in, int ldin, float* out, int B, int C, int H, int W,
                                  hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(in && out && B > 0 && C > 0 && H > 0 && W > 0 && ldin >= C, "hrseg_nhwc_to_nchw: bad arguments");
  const long n = (long)B * H * W;
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, in, ldin, out, B,
                     C, (long)H * W);
  HRSEG_LAUNCH_CHECK("nhwc_to_nchw");
  return 0;
}
