// Split-precision arithmetic on the 16-bit matrix pipe (gfx950): the piece schemes, the on-the-fly operand split, the piece
// products and the PRE-SPLIT activation granule.  Included by every unit that splits or joins: the split-precision convolution
// families (sp_im2col.h, sp_patch.h, conv_sp_*.hip, conv_ws.hip, conv_wgrad_sp.hip) and the BatchNorm unit (bn.hip).
//
// v_mfma_f32_16x16x4_f32 runs at 1/16 of the bf16 MFMA rate.  An fp32 value splits EXACTLY into three bf16
// pieces (8 significand bits each: hi = truncate(x), mid = truncate(x - hi), lo = x - hi - mid), so an fp32
// product is the sum of nine bf16 products of which the three smallest (mid*lo, lo*mid, lo*lo, each below
// 2^-24 of the full product) are dropped: six v_mfma_f32_16x16x32_bf16 with fp32 accumulation per tile and
// K step of 32 do the work of eight fp32 MFMAs in 6/16 of their time ("bf16x3", NS = 3: fp32-grade results).
// NS = 2 keeps two pieces / three products (operand error 2^-16), NS = 1 is plain bf16 inputs with fp32
// accumulation (BASELINE configs[4] arithmetic).  Activations and weights stay fp32 in HBM; the split
// happens on the fly (v_perm_b32 packs two truncated values, v_and + v_sub form the residual).
//
// Measured on MI355X (tools/ubench/bf16_rate.hip): split + MFMA loop, two waves per SIMD: NS=3 298-323 TFLOP/s
// fp32-equivalent (1.8-1.9 PFLOP/s on the matrix pipe), NS=2 535-562, NS=1 1355; the K=16 form
// v_mfma_f32_16x16x16_bf16 runs at HALF the FLOP rate of 16x16x32, so only the K=32 form is used and the
// reduction index runs over 32-wide slabs of the flattened (tap, 16-channel chunk) list.
#pragma once
#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// two floats -> one dword of two bf16 (element 0 in the low half): truncation (exact residual arithmetic)
__device__ __forceinline__ unsigned sp_pack_trunc(float lo, float hi) {
  return __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo), 0x07060302u);
}
// ... round to nearest even (the last piece when fewer than three pieces are kept)
__device__ __forceinline__ unsigned sp_pack_rne(float lo, float hi) {
  const bf16x2 v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float sp_trunc(float x) { return __uint_as_float(__float_as_uint(x) & 0xFFFF0000u); }

// Scheme codes (template parameter NS): 1, 2, 3 = that many bf16 pieces; 4 = "fp16x2": two fp16 pieces (11
// significand bits each: hi = round-toward-zero(x), lo = round-to-nearest(x - hi), 22 bits in all) and the three
// products hi*hi, hi*lo, lo*hi on v_mfma_f32_16x16x32_f16 -- half the matrix work of bf16x3 at 2^-22 operand
// error.  fp16 has 5 exponent bits, so fp16x2 operands are SCALED by a power of two before the split (weights by a
// fixed 2^8, gradients by 2^14 / their measured |max|, see sp_pow2_scale) and the accumulators are scaled back in
// the epilogue; activations are neither scaled nor clamped (exact to 22 bits up to |x| = 65504, Inf / NaN beyond ~1.3e5:
// include/hrseg.h; ops.py range-checks them in deterministic mode).  Elements more than 2^19 below the scaled maximum
// lose their low piece to the subnormal range (absolute error <= 2^-25 after scaling): invisible in a dot product.
constexpr int sp_np(int ns) { return ns == 4 ? 2 : ns; }                       // pieces per operand
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// power-of-two scale that brings the tensor's |max| into [2^14, 2^15) and its inverse (1, 1 for 0 / denormal /
// absent).  `absmax` is the 64-slot array hrseg_bn_bwd_group fills (each slot the max over a share of the blocks).
__device__ __forceinline__ void sp_pow2_scale(const float* absmax, float& scale, float& inv) {
  scale = inv = 1.f;
  if (!absmax) return;
  float m = absmax[threadIdx.x & 63];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  const unsigned e = (__float_as_uint(m) >> 23) & 255u;
  if (e >= 16u && e <= 250u) {
    scale = __uint_as_float((268u - e) << 23);
    inv = __uint_as_float((e - 14u) << 23);
  }
}

__device__ __forceinline__ unsigned sp_pack_f16_rtz(float lo, float hi) {
  return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(lo, hi));
}
__device__ __forceinline__ unsigned sp_pack_f16_rne(float lo, float hi) {
  const f16x2 v = {(_Float16)lo, (_Float16)hi};
  return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float sp_f16_lo(unsigned pk) { return (float)__builtin_bit_cast(f16x2, pk)[0]; }
__device__ __forceinline__ float sp_f16_hi(unsigned pk) { return (float)__builtin_bit_cast(f16x2, pk)[1]; }

// N fp32 (N = 4 or 8, N/2 dwords per piece) -> sp_np(NS) pieces; `sc` scales first (fp16x2 only)
template <int NS, int N>
__device__ __forceinline__ void sp_split(float (&x)[N], unsigned (&out)[sp_np(NS)][N / 2], float sc) {
  if (NS == 4) {
#pragma unroll
    for (int j = 0; j < N; ++j) x[j] *= sc;      // no clamp: NaN propagates, |x| beyond fp16 range ends in Inf / NaN (loud), see hrseg.h
#pragma unroll
    for (int j = 0; j < N / 2; ++j) {
      const unsigned hi = sp_pack_f16_rtz(x[2 * j], x[2 * j + 1]);
      out[0][j] = hi;
      out[1][j] = sp_pack_f16_rne(x[2 * j] - sp_f16_lo(hi), x[2 * j + 1] - sp_f16_hi(hi));
    }
    return;
  }
#pragma unroll
  for (int s = 0; s < sp_np(NS); ++s) {
    const bool last = s == NS - 1;
#pragma unroll
    for (int j = 0; j < N / 2; ++j)
      out[s][j] = (last && NS < 3) ? sp_pack_rne(x[2 * j], x[2 * j + 1]) : sp_pack_trunc(x[2 * j], x[2 * j + 1]);
    if (!last) {
#pragma unroll
      for (int j = 0; j < N; ++j) x[j] -= sp_trunc(x[j]);
    }
  }
}
// 8 fp32 (two f32x4: k = 0..3 and 4..7 of this lane's fragment) -> fragments (128-bit, typed bf16x8 whatever the scheme)
template <int NS>
__device__ __forceinline__ void sp_split8(const f32x4& a, const f32x4& b, bf16x8 (&out)[sp_np(NS)], float sc = 1.f) {
  float x[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  unsigned u[sp_np(NS)][4];
  sp_split<NS, 8>(x, u, sc);
#pragma unroll
  for (int s = 0; s < sp_np(NS); ++s) out[s] = __builtin_bit_cast(bf16x8, (u32x4){u[s][0], u[s][1], u[s][2], u[s][3]});
}
// 4 fp32 -> pieces of 4 elements (8 bytes each): the staging granule
template <int NS>
__device__ __forceinline__ void sp_split4(const f32x4& a, u32x2 (&out)[sp_np(NS)], float sc = 1.f) {
  float x[4] = {a[0], a[1], a[2], a[3]};
  unsigned u[sp_np(NS)][2];
  sp_split<NS, 4>(x, u, sc);
#pragma unroll
  for (int s = 0; s < sp_np(NS); ++s) out[s] = u32x2{u[s][0], u[s][1]};
}

// One fp32 granule (4 channels of a pixel) in PRE-SPLIT fp16x2 form: dwords {hi01, hi23, lo01, lo23} with hi = round-toward-zero
// fp16 of x and lo = round-to-nearest fp16 of (x - hi) -- the two pieces sp_split4<4> above produces on the fly (scale 1), built
// from the same pack primitives, so a convolution that reads a tensor stored this way multiplies the same bits as one that
// splits the fp32 tensor itself.  The writer (hrseg_split_f16x2: BatchNorm apply, z_split) and the readers (hrseg_join_f16x2:
// residual_split; the x_presplit staging of the wave-specialised forward body and of the nine-tap weight gradient) share this
// one contract.
__device__ __forceinline__ u32x4 hrseg_split_f16x2(const f32x4& x) {
  const unsigned h0 = sp_pack_f16_rtz(x[0], x[1]), h1 = sp_pack_f16_rtz(x[2], x[3]);
  return u32x4{h0, h1, sp_pack_f16_rne(x[0] - sp_f16_lo(h0), x[1] - sp_f16_hi(h0)),
               sp_pack_f16_rne(x[2] - sp_f16_lo(h1), x[3] - sp_f16_hi(h1))};
}
// ... and back: hi + lo (exact in fp32: the value the convolutions multiply, the fp32 original rounded to 22 bits)
__device__ __forceinline__ float hrseg_h2f(unsigned bits16) { return (float)__builtin_bit_cast(_Float16, (unsigned short)bits16); }
__device__ __forceinline__ f32x4 hrseg_join_f16x2(const u32x4& g) {
  const unsigned h01 = g[0], h23 = g[1], l01 = g[2], l23 = g[3];
  f32x4 r;
  r[0] = hrseg_h2f(h01 & 0xffffu) + hrseg_h2f(l01 & 0xffffu);
  r[1] = hrseg_h2f(h01 >> 16) + hrseg_h2f(l01 >> 16);
  r[2] = hrseg_h2f(h23 & 0xffffu) + hrseg_h2f(l23 & 0xffffu);
  r[3] = hrseg_h2f(h23 >> 16) + hrseg_h2f(l23 >> 16);
  return r;
}

// acc += W-fragment pieces x X-fragment pieces: the products whose weight is at least 2^-16 (bf16) / 2^-11 (fp16)
// of the full product
template <int NS>
__device__ __forceinline__ f32x4 sp_mma(const bf16x8 (&w)[sp_np(NS)], const bf16x8 (&x)[sp_np(NS)], f32x4 acc) {
  if (NS == 4) {
    const f16x8 w0 = __builtin_bit_cast(f16x8, w[0]), w1 = __builtin_bit_cast(f16x8, w[1]);
    const f16x8 x0 = __builtin_bit_cast(f16x8, x[0]), x1 = __builtin_bit_cast(f16x8, x[1]);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1, x0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0, x1, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(w0, x0, acc, 0, 0, 0);
  }
  if (NS == 3) {   // smallest terms first
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[1], x[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[sp_np(NS) - 1], x[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[0], x[sp_np(NS) - 1], acc, 0, 0, 0);
  }
  if (NS >= 2) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[1 % sp_np(NS)], x[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[0], x[1 % sp_np(NS)], acc, 0, 0, 0);
  }
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[0], x[0], acc, 0, 0, 0);
}

// One product of sp_mma (pr = 0 .. sp_nprod(NS)-1, in sp_mma's order).  The kernels issue the products of a slab
// product-outermost -- all accumulators' first product, then all second ones ... -- so that two MFMAs on the same
// accumulator are never back to back: a dependent 16x16x32 MFMA waits for its predecessor's full latency (twice its
// issue time), and the compiler keeps source order inside an unrolled slab.  Every accumulator still receives its
// products in sp_mma's order, so results are bit-identical to the chained form.
__host__ __device__ constexpr int sp_nprod(int ns) { return ns == 3 ? 6 : ns == 1 ? 1 : 3; }
template <int NS>
__device__ __forceinline__ f32x4 sp_mma_p(int pr, const bf16x8 (&w)[sp_np(NS)], const bf16x8 (&x)[sp_np(NS)], f32x4 acc) {
  int wi = 0, xi = 0;
  if (NS == 3) {
    wi = (pr == 0 || pr == 3) ? 1 : (pr == 1) ? 2 : 0;
    xi = (pr == 0 || pr == 4) ? 1 : (pr == 2) ? 2 : 0;
  } else if (NS != 1) {
    wi = pr == 0 ? 1 : 0;
    xi = pr == 1 ? 1 : 0;
  }
  if (NS == 4)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, w[wi]), __builtin_bit_cast(f16x8, x[xi]), acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[wi], x[xi], acc, 0, 0, 0);
}
