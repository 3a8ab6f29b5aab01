// Sliding-window inference of the device pipelines: hrseg_window_crops cuts the network inputs of all windows of a batch
// straight from the ragged uint8 sources, and hrseg_decode_windows decodes the windows' logits, blended where they overlap,
// to label maps at any size.  Semantics (canvas, origins, the order of the blend's operations): include/hrseg.h.
//
// No canvas-size tensor exists on either side.  A crop pixel is the eval-mode resize of the source to the canvas, evaluated
// at one canvas pixel (the arithmetic of aug_image_eval, resize_u8.h).  The decode keeps the tile shape of
// decode_labels_kernel (decode.hip): grid (blocks, B), striding blocks per image, a tile of 4 output rows x 256 pixels, one
// wave per row, one lane per 4 pixels cut at 4-byte boundaries of the packed label buffer, byte stores only on a row's two
// edges, node table in LDS; the image's window origins (at most 64 per axis) sit in LDS beside it and the blend profile stays
// in global memory (S floats, hot in cache).
//
// An output pixel has 2 x 2 canvas taps, and a canvas pixel is covered by at most 3 x 3 windows, so a channel step fetches
// up to 36 logits where the plain decode fetches 4.  The windows that cover a canvas row (their first index, their number,
// the row inside each and its profile weight) are found once per lane and row tap, those of a canvas column once per pixel
// and column tap; a lane walks its 4 pixels one after the other and the two canvas rows in a rolled loop, so that one pixel's
// column sets and one row's fetches are live at a time (everything unrolled needs 256 registers: DESIGN.md section 9.2), and
// fetches the channels of a group WIN_KU at a time: they share every offset, so each window gives WIN_KU independent loads.
// Only the channels on the decoded path are fetched; a canvas tap whose bilinear weight is 0 (three of four taps where the
// output has the canvas size) is not fetched at all.
#include "decode_common.h"
#include "resize_u8.h"

#define WIN_ORG HRSEG_WINDOW_MAX_ORIGINS
#define WIN_COVER HRSEG_WINDOW_MAX_COVER
#define WIN_DESC 8                                         // int64 entries per image of wdesc
#define WIN_TPB 256
#define WIN_KU 4                                           // channels of a group fetched together by the decode

// ------------------------------------------------------------------------------------------------------------ crops
// grid (blocks, B): the blocks of image m stride over (window of m) x (256-pixel chunk of the S x S plane)
__global__ __launch_bounds__(WIN_TPB) void window_crops_kernel(const u8* __restrict__ src, const long long* __restrict__ desc,
                                                               const long long* __restrict__ wdesc, const int* __restrict__ origins,
                                                               float* __restrict__ x, int S, int nwindows) {
  const int m = blockIdx.y;
  const long long off = desc[4 * m], H = desc[4 * m + 1], W = desc[4 * m + 2], nch = desc[4 * m + 3];
  const long long* wd = wdesc + (size_t)WIN_DESC * m;
  const long long Hc = wd[0], Wc = wd[1], ny = wd[2], nx = wd[3], n0 = wd[4], oo = wd[5];
  if (H < 1 || W < 1 || ny < 1 || nx < 1 || ny > WIN_ORG || nx > WIN_ORG || n0 < 0 || n0 + ny * nx > nwindows) return;
  const size_t plane = (size_t)S * S;
  const long long chunks = (long long)((plane + WIN_TPB - 1) / WIN_TPB), work = ny * nx * chunks;
  const float sy = (float)H / (float)Hc, sx = (float)W / (float)Wc;
  for (long long t = blockIdx.x; t < work; t += gridDim.x) {
    const long long w = t / chunks, q = t - w * chunks;
    const size_t p = (size_t)q * WIN_TPB + threadIdx.x;
    if (p >= plane) continue;
    const int a = (int)(w / nx), b = (int)(w - (long long)a * nx);
    const int i = (int)(p / S), j = (int)(p - (size_t)i * S);
    // (a canvas pixel of a valid table lies inside the canvas; the clamp keeps any other table inside the source)
    const int cy = (int)min((long long)origins[oo + a] + i, Hc - 1), cx = (int)min((long long)origins[oo + ny + b] + j, Wc - 1);
    const Lin iy = lin_index(max(cy, 0), sy, (int)H), ix = lin_index(max(cx, 0), sx, (int)W);
    float* o = x + (size_t)(n0 + w) * 3 * plane + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = (bilinear_u8(src + off, (int)W, (int)nch, nch == 3 ? c : 0, iy, ix) - 0.5f) / 0.5f;
  }
}

// ----------------------------------------------------------------------------------------------------------- decode
// (from here on no contraction: the blend and the channel step round as include/hrseg.h spells them; the crop above keeps the
// default, as augment.hip compiles the same resize)
#pragma clang fp contract(off)

struct DecodeWindowsArgs {
  const float* z[HRSEG_DECODE_MAX_LEVELS];
  int C[HRSEG_DECODE_MAX_LEVELS];
  unsigned node[DEC_NODES];                                // one packed dword per node (decode_common.h)
  int nlevels, root_softmax, S, nwindows;
};

// the windows that cover one canvas coordinate r along one axis: origins first .. first + n - 1 (n <= 3); for each its profile
// weight, its share `win` of the window number and its share `in` of the offset inside a window's plane (rows: base + index *
// nx and coordinate * S, columns: index and coordinate); the weights' sum in ascending order of the origins.
struct WinCover { int n, win[WIN_COVER], in[WIN_COVER]; float w[WIN_COVER], sum; };

__device__ __forceinline__ WinCover win_cover(int r, const int* org, int count, int S, const float* __restrict__ profile, int base,
                                              int mul, int line) {
  int last = 0, hi = count - 1;                            // the last origin <= r (origins ascend from 0)
  while (last < hi) {
    const int mid = (last + hi + 1) >> 1;
    if (org[mid] <= r) last = mid; else hi = mid - 1;
  }
  int first = last;
#pragma unroll
  for (int s = 1; s < WIN_COVER; ++s)
    if (first > 0 && org[first - 1] + S > r) --first;
  WinCover c;
  c.n = (r - org[last] >= 0 && r - org[last] < S) ? last - first + 1 : 0;        // 0: a table that leaves r uncovered
  c.sum = 0.f;
#pragma unroll
  for (int j = 0; j < WIN_COVER; ++j) {
    const int at = r - org[min(first + j, count - 1)];
    const bool in = j < c.n && at >= 0 && at < S;           // (always, with origins that ascend)
    const int inside = in ? at : 0;
    c.win[j] = base + (first + j) * mul;
    c.in[j] = inside * line;
    c.w[j] = in ? profile[inside] : 0.f;
    if (in) c.sum = j == 0 ? c.w[j] : c.sum + c.w[j];
  }
  return c;
}

// blended logits g[kk] of WIN_KU consecutive channels at the canvas pixel (row set R, column set Cc): include/hrseg.h, step 2.
// zc: plane of the first channel in window 0; only nk <= WIN_KU channels exist (the others repeat the last one and are
// dropped by the caller); wstride: floats from one window to the next (64-bit offsets: nwindows * C * S * S is not bounded by
// 2^31).  The channels share every offset, and their fetches from one window are independent: WIN_KU loads in flight.
__device__ __forceinline__ void win_logits(const float* __restrict__ zc, size_t plane, int nk, size_t wstride, const WinCover& R,
                                           const WinCover& Cc, float (&g)[WIN_KU]) {
  const float* zk[WIN_KU];
  float acc[WIN_KU];
#pragma unroll
  for (int kk = 0; kk < WIN_KU; ++kk) {
    zk[kk] = zc + (size_t)min(kk, nk - 1) * plane;
    acc[kk] = 0.f;
  }
#pragma unroll
  for (int ja = 0; ja < WIN_COVER; ++ja) {
    if (ja < R.n) {
#pragma unroll
      for (int jb = 0; jb < WIN_COVER; ++jb) {
        if (jb < Cc.n) {
          const size_t at = (size_t)(R.win[ja] + Cc.win[jb]) * wstride + (size_t)(R.in[ja] + Cc.in[jb]);
          const float w = __fmul_rn(R.w[ja], Cc.w[jb]);
#pragma unroll
          for (int kk = 0; kk < WIN_KU; ++kk) {
            const float t = __fmul_rn(w, zk[kk][at]);
            acc[kk] = (ja == 0 && jb == 0) ? t : __fadd_rn(acc[kk], t);
          }
        }
      }
    }
  }
  const float den = __fmul_rn(R.sum, Cc.sum);
#pragma unroll
  for (int kk = 0; kk < WIN_KU; ++kk) g[kk] = __fdiv_rn(acc[kk], den);
}

// R0 (t == 0) or R1
__device__ __forceinline__ WinCover win_pick(int t, const WinCover& R0, const WinCover& R1) {
  WinCover r;
  r.n = t ? R1.n : R0.n;
  r.sum = t ? R1.sum : R0.sum;
#pragma unroll
  for (int j = 0; j < WIN_COVER; ++j) {
    r.win[j] = t ? R1.win[j] : R0.win[j];
    r.in[j] = t ? R1.in[j] : R0.in[j];
    r.w[j] = t ? R1.w[j] : R0.w[j];
  }
  return r;
}

// (at least 4 waves per SIMD: at most 128 vector registers; without the bound the compiler hoists its way to 256)
template <bool CONF>
__global__ __launch_bounds__(DEC_TPB) __attribute__((amdgpu_waves_per_eu(4, 8))) void decode_windows_kernel(
    DecodeWindowsArgs a, const long long* __restrict__ wdesc, const int* __restrict__ origins, const float* __restrict__ profile,
    const long long* __restrict__ desc, u8* __restrict__ labels, float* __restrict__ conf) {
  __shared__ unsigned tab[DEC_NODES];
  __shared__ int oy[WIN_ORG], ox[WIN_ORG];
  const int b = blockIdx.y, wave = threadIdx.x / HRSEG_WAVE, lane = threadIdx.x & (HRSEG_WAVE - 1);
  const long long off = desc[4 * b], H = desc[4 * b + 1], W = desc[4 * b + 2];
  const long long* wd = wdesc + (size_t)WIN_DESC * b;
  const long long Hc = wd[0], Wc = wd[1], nyl = wd[2], nxl = wd[3], n0l = wd[4], oo = wd[5];
  if (H < 1 || W < 1) return;
  // (block-uniform; the host wrapper refuses such tables: a block never reads a window outside z)
  if (nyl < 1 || nxl < 1 || nyl > WIN_ORG || nxl > WIN_ORG || n0l < 0 || n0l + nyl * nxl > a.nwindows || Hc < a.S || Wc < a.S) return;
  const int ny = (int)nyl, nx = (int)nxl, n0 = (int)n0l, S = a.S;
  if (threadIdx.x < DEC_NODES) tab[threadIdx.x] = a.node[threadIdx.x];
  if (threadIdx.x < ny) oy[threadIdx.x] = origins[oo + threadIdx.x];
  if (threadIdx.x < nx) ox[threadIdx.x] = origins[oo + ny + threadIdx.x];
  __syncthreads();
  // a row may start at any byte: up to 3 pixels of padding in front of it, so (W + 3) pixels cover every alignment
  const long long tiles_x = (W + 3 + DEC_TILE_W - 1) / DEC_TILE_W, tiles_y = (H + DEC_ROWS - 1) / DEC_ROWS;
  const long long ntiles = tiles_x * tiles_y;
  const float sy = (float)Hc / (float)H, sx = (float)Wc / (float)W;
  const size_t plane = (size_t)S * S;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long ty = t / tiles_x, tx = t - ty * tiles_x;
    const long long y = ty * DEC_ROWS + wave;
    if (y >= H) continue;
    const long long row = off + y * W;                                    // first byte of the output row
    const int mis = (int)(((unsigned long long)(uintptr_t)labels + (unsigned long long)row) & 3ull);
    const long long x0 = (tx * HRSEG_WAVE + lane) * DEC_PX - mis;          // labels + row + x0 is 4-byte aligned
    if (x0 >= W || x0 + DEC_PX <= 0) continue;
    const DecLin ly = dec_lin((int)y, sy, (int)Hc);
    const WinCover R0 = win_cover(ly.i0, oy, ny, S, profile, n0, nx, S), R1 = win_cover(ly.i1, oy, ny, S, profile, n0, nx, S);
    const bool row1 = ly.l1 != 0.f;

    // the lane's 4 pixels one after the other (not unrolled: one pixel's column sets and fetches are live at a time)
    unsigned word = 0;                                                    // 4 labels, pixel p in byte p
    float cf0 = 1.f, cf1 = 1.f, cf2 = 1.f, cf3 = 1.f;
#pragma unroll 1
    for (int p = 0; p < DEC_PX; ++p) {
      const long long x = x0 + p;
      if (x < 0 || x >= W) continue;
      const DecLin lx = dec_lin((int)x, sx, (int)Wc);
      const WinCover C0 = win_cover(lx.i0, ox, nx, S, profile, 0, 1, 1), C1 = win_cover(lx.i1, ox, nx, S, profile, 0, 1, 1);
      const bool col1 = lx.l1 != 0.f;
      int start = 0, n = a.C[0];
      float c = 1.f;
      for (int L = 0; L < a.nlevels; ++L) {
        const size_t wstride = (size_t)a.C[L] * plane;
        const bool want_sum = CONF && (L > 0 || a.root_softmax);     // level 0 of a tree model is a sigmoid: no denominator
        float best = -INFINITY, sum = 0.f;
        int arg = 0;
        for (int k0 = 0; k0 < n; k0 += WIN_KU) {                     // WIN_KU channels of the group per step
          const int nk = min(n - k0, WIN_KU);
          const float* __restrict__ zc = a.z[L] + (size_t)(start + k0) * plane;
          float t0[WIN_KU], t1[WIN_KU];                                 // the two canvas rows, blended along x
#pragma unroll
          for (int kk = 0; kk < WIN_KU; ++kk) t0[kk] = t1[kk] = 0.f;
#pragma unroll 1                                                      // (rolled: the fetches of one canvas row are live at a time)
          for (int t = 0; t < (row1 ? 2 : 1); ++t) {
            const WinCover R = win_pick(t, R0, R1);
            float g0[WIN_KU], g1[WIN_KU];
            win_logits(zc, plane, nk, wstride, R, C0, g0);
            if (col1) win_logits(zc, plane, nk, wstride, R, C1, g1);
#pragma unroll
            for (int kk = 0; kk < WIN_KU; ++kk) {
              const float tx = dec_blend2(g0[kk], col1 ? g1[kk] : 0.f, lx.l0, lx.l1);
              t0[kk] = t == 0 ? tx : t0[kk];
              t1[kk] = t == 0 ? t1[kk] : tx;
            }
          }
#pragma unroll
          for (int kk = 0; kk < WIN_KU; ++kk)
            if (kk < nk) dec_step(dec_blend2(t0[kk], t1[kk], ly.l0, ly.l1), k0 + kk, want_sum, best, sum, arg);
        }
        if (CONF) c *= dec_factor(want_sum, best, sum);
        const unsigned e = tab[L * HRSEG_DECODE_MAX_CHANNELS + start + arg];
        const int kids = (int)((e >> 8) & 0xffu);
        if (kids == 0) {
          word |= ((e >> 16) & 0xffu) << (8 * p);
          break;
        }
        start = (int)(e & 0xffu);
        n = kids;
      }
      if (CONF) {
        cf0 = p == 0 ? c : cf0;
        cf1 = p == 1 ? c : cf1;
        cf2 = p == 2 ? c : cf2;
        cf3 = p == 3 ? c : cf3;
      }
    }

    u8* __restrict__ o = labels + row + x0;
    if (x0 >= 0 && x0 + DEC_PX <= W) {
      *reinterpret_cast<unsigned*>(o) = word;
      if (CONF) *reinterpret_cast<f32x4*>(conf + row + x0) = f32x4{cf0, cf1, cf2, cf3};
    } else {
#pragma unroll
      for (int p = 0; p < DEC_PX; ++p) {
        const long long x = x0 + p;
        if (x >= 0 && x < W) {
          o[p] = (u8)(word >> (8 * p));
          if (CONF) conf[row + x] = p == 0 ? cf0 : p == 1 ? cf1 : p == 2 ? cf2 : cf3;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ C ABI
extern "C" int hrseg_window_crops(const unsigned char* src, const long* desc, const long* wdesc, const int* origins, float* x,
                                  int B, int S, int nwindows, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(src && desc && wdesc && origins && x, "hrseg_window_crops: NULL argument");
  HRSEG_CHECK_ARG(B > 0 && B <= 65535, "hrseg_window_crops: B=%d not in 1..65535", B);
  HRSEG_CHECK_ARG(S >= 1 && S <= 32768, "hrseg_window_crops: S=%d not in 1..32768", S);
  HRSEG_CHECK_ARG(nwindows >= B, "hrseg_window_crops: %d windows for %d images", nwindows, B);
  const dim3 grid((unsigned)dec_blocks_per_sample(B), (unsigned)B);
  hipLaunchKernelGGL(window_crops_kernel, grid, dim3(WIN_TPB), 0, (hipStream_t)stream, src, (const long long*)desc,
                     (const long long*)wdesc, origins, x, S, nwindows);
  HRSEG_LAUNCH_CHECK("window_crops");
  hrseg_count(CNT_WINDOW_CROPS);
  return 0;
}

extern "C" int hrseg_decode_windows(int nlevels, const float* const* z, const int* C, const hrseg_decode_tree_t* tree,
                                    const long* wdesc, const int* origins, const float* profile, const long* desc,
                                    unsigned char* labels, float* confidence, int B, int S, int nwindows,
                                    hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(z && C && tree && wdesc && origins && profile && desc && labels, "hrseg_decode_windows: NULL argument");
  HRSEG_CHECK_ARG(B > 0 && B <= 65535, "hrseg_decode_windows: B=%d not in 1..65535", B);
  HRSEG_CHECK_ARG(S >= 1 && S <= 32768, "hrseg_decode_windows: S=%d not in 1..32768", S);
  HRSEG_CHECK_ARG(nwindows >= B, "hrseg_decode_windows: %d windows for %d images", nwindows, B);
  DecodeWindowsArgs a;
  if (const int rc = dec_outputs_and_tree("hrseg_decode_windows", nlevels, C, tree, labels, confidence, a.node, a.C, &a.root_softmax))
    return rc;
  if (const int rc = dec_level_pointers("hrseg_decode_windows", nlevels, z, a.z)) return rc;
  a.nlevels = nlevels;
  a.S = S;
  a.nwindows = nwindows;
  dec_launch(decode_windows_kernel<true>, decode_windows_kernel<false>, confidence, B, stream, a, (const long long*)wdesc, origins,
             profile, (const long long*)desc, labels, confidence);
  HRSEG_LAUNCH_CHECK("decode_windows");
  hrseg_count(CNT_DECODE_WINDOWS);
  return 0;
}
