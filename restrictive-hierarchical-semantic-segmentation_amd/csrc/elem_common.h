// Shared by the NHWC fp32 elementwise units (bn.hip, elem.hip) and the flat-buffer optimiser unit (optim.hip).
//
// Thread mapping used throughout ("pixel lanes x channel quads"): with
// Q = C/4 channel quads, thread t owns quad t % Q for pixel lane t / Q
// (P = 256/Q lanes per block; threads beyond P*Q idle).  Consecutive threads
// read consecutive 16-byte pieces of a pixel row, so a wave covers whole rows.
#pragma once
#include "common.h"

struct Lanes {
  int Q, P, cq, pl;
  bool active;
};
__device__ __forceinline__ Lanes make_lanes(int C) {
  Lanes l;
  l.Q = C >> 2;
  l.P = (l.Q >= 256) ? 1 : 256 / l.Q;
  l.cq = threadIdx.x % l.Q;
  l.pl = threadIdx.x / l.Q;
  l.active = l.pl < l.P;
  return l;
}
static int elem_grid(long npix, int C) {
  const int Q = C / 4, P = (Q >= 256) ? 1 : 256 / Q;
  long blocks = (npix + P - 1) / P;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}
#define FOR_PIXELS(pix, L, npix) \
  for (long pix = (long)blockIdx.x * (L).P + (L).pl; pix < (npix); pix += (long)gridDim.x * (L).P)

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// C > 1024 is not supported by the quad mapping (Q must be <= 256): the widest
// tensor on the path is the UNet 1024-channel concat.
static int check_c(int C, const char* who) {
  HRSEG_CHECK_ARG(C > 0 && C % 4 == 0 && C <= 1024, "%s: C=%d must be a multiple of 4 and <= 1024", who, C);
  return 0;
}

// Flat buffers: 256 threads x 16 bytes, at most 8192 blocks (the grid of the AdamW kernels); n < 4: one block for the tail
static inline int flat_blocks(long n4) {
  long blocks = (n4 + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}
static inline bool al16(const void* q) { return (uintptr_t)q % 16 == 0; }

// An NHWC operand as the 16-byte accesses of the pixel-lane kernels need it: rows of at least C floats that start on
// 16-byte boundaries (ld < C overlaps pixels, ld % 4 != 0 or an odd base is a misaligned access on the device)
static int check_operand(const void* p, int ld, int C, const char* who, const char* what) {
  HRSEG_CHECK_ARG(ld >= C && ld % 4 == 0, "%s: leading dimension %d of %s must be >= C=%d and a multiple of 4", who, ld, what, C);
  HRSEG_CHECK_ARG(al16(p), "%s: %s must be 16-byte aligned", who, what);
  return 0;
}
