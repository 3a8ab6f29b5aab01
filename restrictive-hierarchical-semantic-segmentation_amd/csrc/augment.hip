// Device input pipeline: the reference's per-sample training / evaluation transforms (Data/dataloaders.py:49-70,
// Data/dataset.py:397-470) for a whole batch of ragged uint8 sources, on the GPU.
//
// Image, train mode (2 launches, family "augment_image"):
//  * pass A, one block per 32x32 output tile: bilinear resize (torch, align_corners=False, no antialias) straight
//    from the uint8 source into LDS, with the 12-pixel reflected halo of the 25x25 Gaussian blur; the blur as two
//    1-D passes in LDS (the reference's dense 625-tap conv2d is the outer product of the same taps); the colour-jitter
//    operations that precede contrast in the sample's order; fp32 state out, plus one grayscale partial sum (double)
//    per tile.  No atomics: the partials are reduced in a fixed order by pass B, so the contrast mean is deterministic.
//  * pass B, per output pixel: inverse affine (torchvision _gen_affine_grid + grid_sample nearest), un-flip, read the
//    state, contrast with the per-sample mean and the remaining operations, normalise, fill -1 out of frame.
// Image, eval mode (1 launch): resize + normalise.
//
// Targets (family "augment_targets"): per output pixel the antialiased (or plain bilinear) coverage of every node's
// binary mask, gathered straight from the uint8 label through the 256-entry node bit table, thresholded at 0.5.
// Eval (1 launch): encoded ternary targets written directly.  Train (2 launches): the thresholded node bits of the
// un-warped frame plus a per-block "channel 0 covered" flag, then the warp pass (nearest, un-flip, fill rule:
// channel 0 takes max(mask0) -> 1 if any pixel of it survived the threshold, every other channel 0) and the encode.
#include "common.h"
#include "resize_u8.h"
#include "target_encode.h"

typedef unsigned char u8;
typedef unsigned long long u64;

#define AUG_TILE 32
#define AUG_HALO 12
#define AUG_IN (AUG_TILE + 2 * AUG_HALO)
#define AUG_TPB 256

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

__device__ __forceinline__ float gray3(float r, float g, float b) {
  return __fadd_rn(__fadd_rn(__fmul_rn(0.2989f, r), __fmul_rn(0.587f, g)), __fmul_rn(0.114f, b));
}

// torchvision _rgb2hsv, hue shift (remainder 1), _hsv2rgb
__device__ void adjust_hue(float& r, float& g, float& b, float hue) {
  const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
  const bool eqc = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eqc ? 1.f : maxc);
  const float crd = eqc ? 1.f : cr;
  const float rc = (maxc - r) / crd, gc = (maxc - g) / crd, bc = (maxc - b) / crd;
  const float hr = (maxc == r) ? (bc - gc) : 0.f;
  const float hg = (maxc == g && maxc != r) ? ((2.f + rc) - bc) : 0.f;
  const float hb = (maxc != g && maxc != r) ? ((4.f + gc) - rc) : 0.f;
  float h = fmodf(((hr + hg) + hb) / 6.f + 1.f, 1.f);
  h = h + hue;
  h = h - floorf(h);
  const float v = maxc;
  const float h6 = h * 6.f;
  const float fi = floorf(h6);
  const float f = h6 - fi;
  int i = ((int)fi) % 6;
  if (i < 0) i += 6;
  const float p = clamp01(v * (1.f - s));
  const float q = clamp01(v * (1.f - s * f));
  const float t = clamp01(v * (1.f - s * (1.f - f)));
  switch (i) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}

// ColorJitter operation `op` (0 brightness, 1 contrast, 2 saturation, 3 hue); blend = clamp(f*a + (1-f)*m, 0, 1)
__device__ __forceinline__ void jitter_op(int op, float& r, float& g, float& b, const float* __restrict__ P, float mean) {
  if (op == 0) {
    const float f = P[HRSEG_AUG_P_BRIGHT];
    r = clamp01(f * r); g = clamp01(f * g); b = clamp01(f * b);
  } else if (op == 1) {
    const float f = P[HRSEG_AUG_P_CONTRAST], m = P[HRSEG_AUG_P_CONTRAST + 1] * mean;
    r = clamp01(f * r + m); g = clamp01(f * g + m); b = clamp01(f * b + m);
  } else if (op == 2) {
    const float f = P[HRSEG_AUG_P_SAT], om = P[HRSEG_AUG_P_SAT + 1];
    const float m = om * gray3(r, g, b);
    r = clamp01(f * r + m); g = clamp01(f * g + m); b = clamp01(f * b + m);
  } else {
    adjust_hue(r, g, b, P[HRSEG_AUG_P_HUE]);
  }
}

__device__ __forceinline__ int reflect_clamp(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return min(max(i, 0), n - 1);         // (halo rows / columns no valid output reads)
}

// output pixel (i, j) -> pixel (si, sj) of the un-warped, un-flipped frame; false = out of frame
__device__ __forceinline__ bool warp_source(const float* __restrict__ P, int S, int i, int j, int& si, int& sj) {
  const int flags = (int)P[HRSEG_AUG_P_FLAGS];
  si = i;
  sj = j;
  if (flags & HRSEG_AUG_WARP) {
    const float* t = P + HRSEG_AUG_P_THETA;      // rescaled theta^T: x' = x t0 + y t2 + t4, y' = x t1 + y t3 + t5
    const float xb = (float)j - 0.5f * (float)S + 0.5f, yb = (float)i - 0.5f * (float)S + 0.5f;
    const float gx = __fadd_rn(__fadd_rn(__fmul_rn(xb, t[0]), __fmul_rn(yb, t[2])), t[4]);
    const float gy = __fadd_rn(__fadd_rn(__fmul_rn(xb, t[1]), __fmul_rn(yb, t[3])), t[5]);
    const float half = 0.5f * (float)S;
    const float ix = __fsub_rn(__fmul_rn(gx + 1.f, half), 0.5f), iy = __fsub_rn(__fmul_rn(gy + 1.f, half), 0.5f);
    const float rx = rintf(ix), ry = rintf(iy);
    if (!(rx >= 0.f && rx <= (float)(S - 1) && ry >= 0.f && ry <= (float)(S - 1))) return false;
    sj = (int)rx;
    si = (int)ry;
  }
  if (flags & HRSEG_AUG_HFLIP) sj = S - 1 - sj;
  if (flags & HRSEG_AUG_VFLIP) si = S - 1 - si;
  return true;
}

// ------------------------------------------------------------------------------------------------------------ image
__global__ __launch_bounds__(AUG_TPB) void aug_image_pass_a(const u8* __restrict__ src, const long long* __restrict__ desc,
                                                            const float* __restrict__ params, float* __restrict__ state,
                                                            double* __restrict__ partials, int S, int tiles_x, int ntiles) {
  __shared__ float in[3][AUG_IN][AUG_IN + 1];
  __shared__ float hb[3][AUG_IN][AUG_TILE + 1];
  __shared__ double red[AUG_TPB / HRSEG_WAVE];
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const int ty0 = (tile / tiles_x) * AUG_TILE, tx0 = (tile % tiles_x) * AUG_TILE;
  const long long off = desc[4 * b], H = desc[4 * b + 1], W = desc[4 * b + 2], nch = desc[4 * b + 3];
  const u8* s = src + off;
  const float* P = params + (size_t)b * HRSEG_AUG_PARAMS;
  const float sy = (float)H / (float)S, sx = (float)W / (float)S;
  for (int e = tid; e < AUG_IN * AUG_IN; e += AUG_TPB) {
    const int ly = e / AUG_IN, lx = e - ly * AUG_IN;
    const Lin iy = lin_index(reflect_clamp(ty0 - AUG_HALO + ly, S), sy, (int)H);
    const Lin ix = lin_index(reflect_clamp(tx0 - AUG_HALO + lx, S), sx, (int)W);
#pragma unroll
    for (int c = 0; c < 3; ++c) in[c][ly][lx] = bilinear_u8(s, (int)W, (int)nch, nch == 3 ? c : 0, iy, ix);
  }
  __syncthreads();
  const float* taps = P + HRSEG_AUG_P_TAPS;
  for (int e = tid; e < 3 * AUG_IN * AUG_TILE; e += AUG_TPB) {
    const int c = e / (AUG_IN * AUG_TILE), r = e - c * (AUG_IN * AUG_TILE), ly = r / AUG_TILE, ox = r - ly * AUG_TILE;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 25; ++k) acc += taps[k] * in[c][ly][ox + k];
    hb[c][ly][ox] = acc;
  }
  __syncthreads();
  const int order[4] = {(int)P[HRSEG_AUG_P_ORDER], (int)P[HRSEG_AUG_P_ORDER + 1], (int)P[HRSEG_AUG_P_ORDER + 2],
                        (int)P[HRSEG_AUG_P_ORDER + 3]};
  double gsum = 0.0;
  const size_t plane = (size_t)S * S;
  for (int p = tid; p < AUG_TILE * AUG_TILE; p += AUG_TPB) {
    const int oy = p / AUG_TILE, ox = p - oy * AUG_TILE, gy = ty0 + oy, gx = tx0 + ox;
    if (gy >= S || gx >= S) continue;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < 25; ++k) acc += taps[k] * hb[c][oy + k][ox];
      v[c] = acc;
    }
    for (int k = 0; k < 4 && order[k] != 1; ++k) jitter_op(order[k], v[0], v[1], v[2], P, 0.f);
    gsum += (double)gray3(v[0], v[1], v[2]);
    float* o = state + (size_t)b * 3 * plane + (size_t)gy * S + gx;
    o[0] = v[0];
    o[plane] = v[1];
    o[2 * plane] = v[2];
  }
  gsum = wave_sum_d(gsum);
  if ((tid & (HRSEG_WAVE - 1)) == 0) red[tid / HRSEG_WAVE] = gsum;
  __syncthreads();
  if (tid == 0) partials[(size_t)b * ntiles + tile] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(AUG_TPB) void aug_image_pass_b(const float* __restrict__ state, const double* __restrict__ partials,
                                                            const float* __restrict__ params, float* __restrict__ x, int S,
                                                            int ntiles) {
  __shared__ double red[AUG_TPB / HRSEG_WAVE];
  const int b = blockIdx.y, tid = threadIdx.x;
  double acc = 0.0;
  for (int t = tid; t < ntiles; t += AUG_TPB) acc += partials[(size_t)b * ntiles + t];     // fixed order: deterministic
  acc = wave_sum_d(acc);
  if ((tid & (HRSEG_WAVE - 1)) == 0) red[tid / HRSEG_WAVE] = acc;
  __syncthreads();
  const float mean = (float)((((red[0] + red[1]) + red[2]) + red[3]) / ((double)S * S));
  const long p = (long)blockIdx.x * AUG_TPB + tid;
  const size_t plane = (size_t)S * S;
  if (p >= (long)plane) return;
  const int i = (int)(p / S), j = (int)(p - (long)i * S);
  const float* P = params + (size_t)b * HRSEG_AUG_PARAMS;
  float* o = x + (size_t)b * 3 * plane + p;
  int si, sj;
  if (!warp_source(P, S, i, j, si, sj)) {
    o[0] = o[plane] = o[2 * plane] = -1.f;
    return;
  }
  const float* st = state + (size_t)b * 3 * plane + (size_t)si * S + sj;
  float v0 = st[0], v1 = st[plane], v2 = st[2 * plane];
  bool after = false;
  for (int k = 0; k < 4; ++k) {
    const int op = (int)P[HRSEG_AUG_P_ORDER + k];
    if (op == 1) after = true;
    if (after) jitter_op(op, v0, v1, v2, P, mean);
  }
  o[0] = (v0 - 0.5f) / 0.5f;
  o[plane] = (v1 - 0.5f) / 0.5f;
  o[2 * plane] = (v2 - 0.5f) / 0.5f;
}

__global__ __launch_bounds__(AUG_TPB) void aug_image_eval(const u8* __restrict__ src, const long long* __restrict__ desc,
                                                          float* __restrict__ x, int S) {
  const int b = blockIdx.y;
  const long p = (long)blockIdx.x * AUG_TPB + threadIdx.x;
  const size_t plane = (size_t)S * S;
  if (p >= (long)plane) return;
  const int i = (int)(p / S), j = (int)(p - (long)i * S);
  const long long off = desc[4 * b], H = desc[4 * b + 1], W = desc[4 * b + 2], nch = desc[4 * b + 3];
  const Lin iy = lin_index(i, (float)H / (float)S, (int)H), ix = lin_index(j, (float)W / (float)S, (int)W);
  float* o = x + (size_t)b * 3 * plane + p;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c * plane] = (bilinear_u8(src + off, (int)W, (int)nch, nch == 3 ? c : 0, iy, ix) - 0.5f) / 0.5f;
}

// ---------------------------------------------------------------------------------------------------------- targets
// torch _upsample_bilinear2d_aa weights of one output coordinate (HelperInterpLinear, antialias=True)
struct AaSpan { int lo, n; float center, invscale, total; };
__device__ __forceinline__ float aa_filter(float x) {
  if (x < 0.f) x = -x;
  return x < 1.f ? 1.f - x : 0.f;
}
__device__ __forceinline__ float aa_weight(const AaSpan& a, int k) {
  return aa_filter((float)(((double)((float)(k + a.lo) - a.center) + 0.5) * (double)a.invscale));
}
__device__ __forceinline__ AaSpan aa_span(int dst, int in, int out) {
  const float scale = (float)in / (float)out;
  const float support = scale >= 1.f ? scale : 1.f;
  AaSpan a;
  a.center = scale * ((float)dst + 0.5f);
  a.invscale = scale >= 1.f ? 1.f / scale : 1.f;
  a.lo = max((int)((double)(a.center - support) + 0.5), 0);
  a.n = min((int)((double)(a.center + support) + 0.5), in) - a.lo;
  float t = 0.f;
  for (int k = 0; k < a.n; ++k) t += aa_weight(a, k);
  a.total = t;
  return a;
}

// One tap of weight w on the pixel value v: every accumulator of the chunk that starts at channel c0 (written out in the
// kernel's own scope: through a function taking the arrays by reference the 64-wide instance needs 154 registers, not 109)
#define AUG_COVER_TAP(v, w)                                                   \
  do {                                                                        \
    const u64 nb_ = lut[v] >> c0;                                             \
    _Pragma("unroll") for (int c = 0; c < NC; ++c) acc[c] += ((nb_ >> c) & 1ull) ? (w) : 0.f; \
    if constexpr (PARTIAL) {                                                  \
      const u64 mb_ = mlut[v] >> c0;                                          \
      _Pragma("unroll") for (int c = 0; c < NC; ++c) accm[c] += ((mb_ >> c) & 1ull) ? (w) : 0.f; \
    }                                                                         \
  } while (0)

// coverage of every node at output pixel p of the un-warped frame, thresholded (< 0.5 -> 0); direct: encode and
// write y, else write the bits and this block's "channel 0 covered anywhere" flag.
// PARTIAL (partial labels, include/hrseg.h): a second accumulator per channel, may[c], adds the same weights in the same
// order over the pixels where the node is on OR unknown, so may[c] >= on[c] and with unk_lut all zero the two are
// bit-equal; UNK = (may >= 0.5) and not (on >= 0.5).  The channels go in chunks of NC, each chunk a walk of its own over
// the footprint (one chunk wherever C <= NC); the bits of a pixel are two words, ON then UNK.
template <int NC, bool PARTIAL>
__global__ __launch_bounds__(AUG_TPB) void aug_targets_cover(const u8* __restrict__ label, const long long* __restrict__ desc,
                                                             const u64* __restrict__ on_lut, const u64* __restrict__ unk_lut,
                                                             TargetParents pr, float* __restrict__ y, u64* __restrict__ bits,
                                                             int* __restrict__ flags, int C, int S, int antialias, int direct) {
  __shared__ u64 lut[256];
  __shared__ u64 mlut[PARTIAL ? 256 : 1];
  lut[threadIdx.x] = on_lut[threadIdx.x];
  if constexpr (PARTIAL) mlut[threadIdx.x] = on_lut[threadIdx.x] | unk_lut[threadIdx.x];
  __syncthreads();
  const int b = blockIdx.y;
  const long p = (long)blockIdx.x * AUG_TPB + threadIdx.x;
  const size_t plane = (size_t)S * S;
  const bool valid = p < (long)plane;
  u64 m = 0, may = 0;
  if (valid) {
    const int i = (int)(p / S), j = (int)(p - (long)i * S);
    const long long off = desc[4 * b], H = desc[4 * b + 1], W = desc[4 * b + 2];
    const u8* l = label + off;
    for (int c0 = 0; c0 < (PARTIAL ? C : 1); c0 += NC) {
      float acc[NC], accm[PARTIAL ? NC : 1];
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] = 0.f;
      if constexpr (PARTIAL) {
#pragma unroll
        for (int c = 0; c < NC; ++c) accm[c] = 0.f;
      }
      if (antialias) {
        const AaSpan ay = aa_span(i, (int)H, S), ax = aa_span(j, (int)W, S);
        for (int ky = 0; ky < ay.n; ++ky) {
          const float wy = ay.total != 0.f ? aa_weight(ay, ky) / ay.total : aa_weight(ay, ky);
          if (wy == 0.f) continue;
          const u8* row = l + (long)(ay.lo + ky) * W + ax.lo;
          for (int kx = 0; kx < ax.n; ++kx) {
            const float wx = ax.total != 0.f ? aa_weight(ax, kx) / ax.total : aa_weight(ax, kx);
            const float w = wy * wx;
            const u8 v = row[kx];
            AUG_COVER_TAP(v, w);
          }
        }
      } else {
        const Lin iy = lin_index(i, (float)H / (float)S, (int)H), ix = lin_index(j, (float)W / (float)S, (int)W);
        const int ys[2] = {iy.i0, iy.i1}, xs[2] = {ix.i0, ix.i1};
        const float wys[2] = {iy.l0, iy.l1}, wxs[2] = {ix.l0, ix.l1};
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const float w = wys[a] * wxs[q];
            const u8 v = l[(long)ys[a] * W + xs[q]];
            AUG_COVER_TAP(v, w);
          }
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (c0 + c < C && acc[c] >= 0.5f) m |= 1ull << (c0 + c);
        if constexpr (PARTIAL)
          if (c0 + c < C && accm[c] >= 0.5f) may |= 1ull << (c0 + c);
      }
    }
    const u64 unk = may & ~m;
    if (direct) encode_write(m, unk, pr, y + (size_t)b * C * plane + p, C, plane);
    else if (PARTIAL) {
      bits[2 * ((size_t)b * plane + p)] = m;
      bits[2 * ((size_t)b * plane + p) + 1] = unk;
    } else bits[(size_t)b * plane + p] = m;
  }
  if (!direct) {
    const int any = __syncthreads_or((int)(m & 1ull));
    if (threadIdx.x == 0) flags[(size_t)b * gridDim.x + blockIdx.x] = any;
  }
}

#undef AUG_COVER_TAP

// the warp moves the thresholded sets; out of frame: ON = {channel 0} if channel 0 is covered anywhere in the image, UNK
// empty (the reference's fill), or with fill_unknown (PARTIAL only) ON empty and UNK every channel
template <bool PARTIAL>
__global__ __launch_bounds__(AUG_TPB) void aug_targets_warp(const u64* __restrict__ bits, const int* __restrict__ flags,
                                                            const float* __restrict__ params, TargetParents pr,
                                                            float* __restrict__ y, int C, int S, int fill_unknown) {
  const int b = blockIdx.y, nblk = gridDim.x;
  int any = 0;
  for (int t = threadIdx.x; t < nblk; t += AUG_TPB) any |= flags[(size_t)b * nblk + t];
  any = __syncthreads_or(any);
  const long p = (long)blockIdx.x * AUG_TPB + threadIdx.x;
  const size_t plane = (size_t)S * S;
  if (p >= (long)plane) return;
  const int i = (int)(p / S), j = (int)(p - (long)i * S);
  int si, sj;
  const bool inside = warp_source(params + (size_t)b * HRSEG_AUG_PARAMS, S, i, j, si, sj);
  const size_t src = (size_t)b * plane + (size_t)si * S + sj;
  u64 m, unk = 0;
  if (PARTIAL) {
    const u64 all = C == 64 ? ~0ull : (1ull << C) - 1;
    m = inside ? bits[2 * src] : (u64)(!fill_unknown && any ? 1 : 0);
    unk = inside ? bits[2 * src + 1] : (fill_unknown ? all : 0ull);
  } else {
    m = inside ? bits[src] : (u64)(any ? 1 : 0);
  }
  encode_write(m, unk, pr, y + (size_t)b * C * plane + p, C, plane);
}

// ------------------------------------------------------------------------------------------------------------ C ABI
static size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
static int aug_tiles(int S) { return ceil_div(S, AUG_TILE); }

extern "C" int hrseg_augment_workspace(int B, int S, size_t* image_bytes, size_t* target_bytes) {
  HRSEG_CHECK_ARG(B > 0 && S > 0 && image_bytes && target_bytes, "hrseg_augment_workspace: bad arguments");
  const size_t plane = (size_t)S * S;
  const int nt = aug_tiles(S), nblk = ceil_div((long)plane, AUG_TPB);
  *image_bytes = align256((size_t)B * 3 * plane * sizeof(float)) + align256((size_t)B * nt * nt * sizeof(double));
  *target_bytes = align256((size_t)B * plane * sizeof(u64)) + align256((size_t)B * nblk * sizeof(int));
  return 0;
}

extern "C" int hrseg_augment_image(const unsigned char* src, const long* desc, const float* params, float* x, int B, int S,
                                   int train, void* work, size_t work_bytes, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(src && desc && x && B > 0 && B <= 65535 && S > 0, "hrseg_augment_image: bad arguments");
  const hipStream_t st = (hipStream_t)stream;
  const long plane = (long)S * S;
  const dim3 grid_px((unsigned)ceil_div(plane, AUG_TPB), (unsigned)B);
  if (!train) {
    hipLaunchKernelGGL(aug_image_eval, grid_px, dim3(AUG_TPB), 0, st, src, (const long long*)desc, x, S);
    HRSEG_LAUNCH_CHECK("augment_image_eval");
    hrseg_count(CNT_AUG_IMAGE);
    return 0;
  }
  HRSEG_CHECK_ARG(params && work, "hrseg_augment_image: train mode needs params and a workspace");
  HRSEG_CHECK_ARG(S > AUG_HALO, "hrseg_augment_image: S=%d too small for the 25x25 reflect-padded blur", S);
  size_t need_i, need_t;
  hrseg_augment_workspace(B, S, &need_i, &need_t);
  HRSEG_CHECK_ARG(work_bytes >= need_i, "hrseg_augment_image: workspace %zu bytes, needs %zu", work_bytes, need_i);
  const int nt = aug_tiles(S);
  float* state = (float*)work;
  double* partials = (double*)((char*)work + align256((size_t)B * 3 * plane * sizeof(float)));
  hipLaunchKernelGGL(aug_image_pass_a, dim3((unsigned)(nt * nt), (unsigned)B), dim3(AUG_TPB), 0, st, src,
                     (const long long*)desc, params, state, partials, S, nt, nt * nt);
  HRSEG_LAUNCH_CHECK("augment_image_pass_a");
  hipLaunchKernelGGL(aug_image_pass_b, grid_px, dim3(AUG_TPB), 0, st, state, partials, params, x, S, nt * nt);
  HRSEG_LAUNCH_CHECK("augment_image_pass_b");
  hrseg_count(CNT_AUG_IMAGE, 2);
  return 0;
}

extern "C" int hrseg_augment_workspace_partial(int B, int S, size_t* target_bytes) {
  HRSEG_CHECK_ARG(B > 0 && S > 0 && target_bytes, "hrseg_augment_workspace_partial: bad arguments");
  const size_t plane = (size_t)S * S;
  *target_bytes = align256((size_t)B * plane * 2 * sizeof(u64)) + align256((size_t)B * ceil_div((long)plane, AUG_TPB) * sizeof(int));
  return 0;
}

// both target entry points: `name` is the one that was called.  Coverage instances: 16 accumulators per set where C <= 16;
// above that the fully labelled path keeps all 64 channels in one walk, the partial path walks once per 32 channels
// (2 x 32 accumulators: DESIGN.md section 25 has the register counts behind the choice).
static int augment_targets(const char* name, const unsigned char* label, const long* desc, const u64* on_lut, const u64* unk_lut,
                           bool partial, const int* parent, const float* params, float* y, int B, int C, int S, int warp,
                           int antialias, int fill_unknown, void* work, size_t work_bytes, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(label && desc && on_lut && (!partial || unk_lut) && parent && y && B > 0 && B <= 65535 && S > 0,
                  "%s: bad arguments", name);
  HRSEG_CHECK_ARG(C >= 1 && C <= 64, "%s: C=%d not in 1..64", name, C);
  TargetParents pr;
  const int bad = target_parents(parent, C, pr);
  HRSEG_CHECK_ARG(bad < 0, "%s: parent[%d]=%d out of range", name, bad, parent[bad < 0 ? 0 : bad]);
  const hipStream_t st = (hipStream_t)stream;
  const long plane = (long)S * S;
  const dim3 grid_px((unsigned)ceil_div(plane, AUG_TPB), (unsigned)B);
  u64* bits = nullptr;
  int* flags = nullptr;
  if (warp) {
    HRSEG_CHECK_ARG(params && work, "%s: the warp needs params and a workspace", name);
    size_t need_i, need_t;
    if (partial) hrseg_augment_workspace_partial(B, S, &need_t);
    else hrseg_augment_workspace(B, S, &need_i, &need_t);
    HRSEG_CHECK_ARG(work_bytes >= need_t, "%s: workspace %zu bytes, needs %zu", name, work_bytes, need_t);
    bits = (u64*)work;
    flags = (int*)((char*)work + align256((size_t)B * plane * (partial ? 2 : 1) * sizeof(u64)));
  }
  const long long* d = (const long long*)desc;
  const int direct = warp ? 0 : 1;
#define COVER(NC, P) \
  hipLaunchKernelGGL((aug_targets_cover<NC, P>), grid_px, dim3(AUG_TPB), 0, st, label, d, on_lut, unk_lut, pr, y, bits, flags, C, S, \
                     antialias, direct)
  if (partial) {
    if (C <= 16) COVER(16, true);
    else COVER(32, true);
  } else {
    if (C <= 16) COVER(16, false);
    else COVER(64, false);
  }
#undef COVER
  HRSEG_LAUNCH_CHECK("augment_targets_cover");
  if (warp) {
    if (partial)
      hipLaunchKernelGGL(aug_targets_warp<true>, grid_px, dim3(AUG_TPB), 0, st, bits, flags, params, pr, y, C, S, fill_unknown);
    else
      hipLaunchKernelGGL(aug_targets_warp<false>, grid_px, dim3(AUG_TPB), 0, st, bits, flags, params, pr, y, C, S, 0);
    HRSEG_LAUNCH_CHECK("augment_targets_warp");
  }
  hrseg_count(CNT_AUG_TARGETS, warp ? 2 : 1);
  return 0;
}

extern "C" int hrseg_augment_targets(const unsigned char* label, const long* desc, const unsigned long long* on_lut,
                                     const int* parent, const float* params, float* y, int B, int C, int S, int warp,
                                     int antialias, void* work, size_t work_bytes, hrseg_stream_t stream) {
  return augment_targets("hrseg_augment_targets", label, desc, on_lut, nullptr, false, parent, params, y, B, C, S, warp, antialias,
                         0, work, work_bytes, stream);
}

extern "C" int hrseg_augment_targets_partial(const unsigned char* label, const long* desc, const unsigned long long* on_lut,
                                             const unsigned long long* unk_lut, const int* parent, const float* params, float* y,
                                             int B, int C, int S, int warp, int antialias, int fill_unknown, void* work,
                                             size_t work_bytes, hrseg_stream_t stream) {
  return augment_targets("hrseg_augment_targets_partial", label, desc, on_lut, unk_lut, true, parent, params, y, B, C, S, warp,
                         antialias, fill_unknown, work, work_bytes, stream);
}
