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
    for (int j = 0; j < 4; ++j) m[j] = fmaxf(fmaxf(m[j], v1[j]), fmaxf(v2[j], v3[j]));
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
    if (relu) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
    }
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
    if (a.relu) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
    }
    st4(a.out + pix * a.ldo + 4 * L.cq, v);
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

// --------------------------------------------------------------------------- small glue
__global__ __launch_bounds__(256) void add_kernel(const float* __restrict__ a, int lda, const float* __restrict__ b,
                                                  int ldb, float* __restrict__ out, int ldo, int relu, long npix,
                                                  int C) {
  const Lanes L = make_lanes(C);
  if (!L.active) return;
  FOR_PIXELS(pix, L, npix) {
    f32x4 v = ld4(a + pix * lda + 4 * L.cq) + ld4(b + pix * ldb + 4 * L.cq);
    if (relu) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
    }
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
      for (int j = 0; j < 4; ++j) amax = fmaxf(amax, (v[j] != v[j]) ? __builtin_inff() : fabsf(v[j]));
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
  FuseSumArgs a{};
  a.n_same = n_same; a.n_low = n_low;
  for (int i = 0; i < n_same; ++i) {
    HRSEG_CHECK_ARG(same[i] && ld_same[i] >= C && ld_same[i] % 4 == 0, "hrseg_fuse_sum: bad same-resolution term %d", i);
    a.same[i] = same[i]; a.ld_same[i] = ld_same[i];
  }
  for (int j = 0; j < n_low; ++j) {
    HRSEG_CHECK_ARG(low[j] && ld_low[j] >= C && ld_low[j] % 4 == 0 && Hi[j] > 0 && Wi[j] > 0, "hrseg_fuse_sum: bad low-resolution term %d", j);
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

extern "C" int hrseg_add(const float* a, int lda, const float* b, int ldb, float* out, int ldo, int relu, long npix,
                         int C, hrseg_stream_t stream) {
  if (int e = check_c(C, "hrseg_add")) return e;
  HRSEG_CHECK_ARG(a && b && out && npix > 0, "hrseg_add: bad arguments");
  hipLaunchKernelGGL(add_kernel, dim3(elem_grid(npix, C)), dim3(256), 0, (hipStream_t)stream, a, lda, b, ldb, out, ldo,
                     relu, npix, C);
  HRSEG_LAUNCH_CHECK("add");
  return 0;
}

extern "C" int hrseg_copy(const float* in, int ldin, float* out, int ldout, int accumulate, long npix, int C,
                          hrseg_stream_t stream) {
  if (int e = check_c(C, "hrseg_copy")) return e;
  HRSEG_CHECK_ARG(in && out && npix > 0, "hrseg_copy: bad arguments");
  hipLaunchKernelGGL(copy_kernel, dim3(elem_grid(npix, C)), dim3(256), 0, (hipStream_t)stream, in, ldin, out, ldout,
                     accumulate, npix, C);
  HRSEG_LAUNCH_CHECK("copy");
  return 0;
}

extern "C" int hrseg_relu_bwd(const float* dz, int lddz, const float* z, int ldz, float* dx, int lddx, long npix,
                              int C, hrseg_stream_t stream) {
  if (int e = check_c(C, "hrseg_relu_bwd")) return e;
  HRSEG_CHECK_ARG(dz && z && dx && npix > 0, "hrseg_relu_bwd: bad arguments");
  hipLaunchKernelGGL(relu_bwd_kernel, dim3(elem_grid(npix, C)), dim3(256), 0, (hipStream_t)stream, dz, lddz, z, ldz,
                     dx, lddx, npix, C);
  HRSEG_LAUNCH_CHECK("relu_bwd");
  return 0;
}

extern "C" int hrseg_absmax(const float* x, int ldx, long npix, int C, float* out64, hrseg_stream_t stream) {
  if (int e = check_c(C, "hrseg_absmax")) return e;
  HRSEG_CHECK_ARG(x && out64 && npix > 0 && ldx >= C, "hrseg_absmax: bad arguments");
  hipLaunchKernelGGL(absmax_kernel, dim3(elem_grid(npix, C)), dim3(256), 0, (hipStream_t)stream, x, ldx, npix, C, out64);
  HRSEG_LAUNCH_CHECK("absmax");
  return 0;
}

extern "C" int hrseg_nchw_to_nhwc(const float* in, float* out, int ldout, int B, int C, int H, int W,
                                  hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(in && out && B > 0 && C > 0 && ldout >= C, "hrseg_nchw_to_nhwc: bad arguments");
  const long n = (long)B * H * W;
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, in, out, ldout, B,
                     C, (long)H * W);
  HRSEG_LAUNCH_CHECK("nchw_to_nhwc");
  return 0;
}

extern "C" int hrseg_nhwc_to_nchw(const float* in, int ldin, float* out, int B, int C, int H, int W,
                                  hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(in && out && B > 0 && C > 0 && ldin >= C, "hrseg_nhwc_to_nchw: bad arguments");
  const long n = (long)B * H * W;
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, in, ldin, out, B,
                     C, (long)H * W);
  HRSEG_LAUNCH_CHECK("nhwc_to_nchw");
  return 0;
}
