// The eval-mode resize of a uint8 source, shared by augment.hip (whole images) and windows.hip (window crops of a canvas).
#pragma once
#include "common.h"

typedef unsigned char u8;

// torch upsample_bilinear2d (align_corners=False) source index and weights of one output coordinate
struct Lin { int i0, i1; float l0, l1; };
__device__ __forceinline__ Lin lin_index(int dst, float scale, int in) {
  float real = __fsub_rn(__fmul_rn(scale, (float)dst + 0.5f), 0.5f);
  if (real < 0.f) real = 0.f;
  Lin r;
  r.i0 = (int)real;
  const float lam = fminf(fmaxf(real - (float)r.i0, 0.f), 1.f);
  r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
  r.l1 = lam;
  r.l0 = 1.f - lam;
  return r;
}

// one channel of a uint8 source (HWC for 3 channels, HW for 1) at output pixel (ly, lx) of the resize, in [0, 1]
__device__ __forceinline__ float bilinear_u8(const u8* __restrict__ s, int W, int nch, int c, const Lin& ly, const Lin& lx) {
  const float p00 = (float)s[((long)ly.i0 * W + lx.i0) * nch + c] / 255.f;
  const float p01 = (float)s[((long)ly.i0 * W + lx.i1) * nch + c] / 255.f;
  const float p10 = (float)s[((long)ly.i1 * W + lx.i0) * nch + c] / 255.f;
  const float p11 = (float)s[((long)ly.i1 * W + lx.i1) * nch + c] / 255.f;
  const float t0 = __fadd_rn(__fmul_rn(p00, lx.l0), __fmul_rn(p01, lx.l1));
  const float t1 = __fadd_rn(__fmul_rn(p10, lx.l0), __fmul_rn(p11, lx.l1));
  return __fadd_rn(__fmul_rn(t0, ly.l0), __fmul_rn(t1, ly.l1));
}
