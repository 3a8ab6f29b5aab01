// Split-precision weight gradients (tap-per-block and nine-tap): kernel instances + launchers.
#include "conv_common.h"
#include "sp_arith.h"

// --------------------------------------------------------------------------- weight gradient
// dW[co][t][ci] += sum_pix dy[pix][co] * x[pix_t][ci] on the bf16 matrix pipe.  Block = (tap, 16*TN couts,
// 16*TK cins, pixel range) as in wgrad_body; a stage is 128 pixels, 32 per wave = one K step of the MFMA.
// Both operands run over PIXELS in the reduction index, which is the strided direction of NHWC memory, so
// both tiles are staged (split on the fly) as [pixel][channel] bf16 images in LDS and read back TRANSPOSED
// with ds_read_b64_tr_b16: a 16-lane group fetches 4 pixel rows x 16 channels and every lane receives its
// channel's 4 pixels.  Two such reads make one K=32 fragment; lane group g takes pixels 4g..4g+3 and
// 16+4g..16+4g+3 of the wave's 32 (the same permutation on both operands), which keeps the two groups of
// a 32-lane half on different bank rows when the row stride is an odd multiple of 32 bytes.
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ s16x4 sp_tr_read(const unsigned char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(p));
}

constexpr int sp_row_stride(int channels) {       // bytes per pixel row: 2*channels rounded up to 32 * odd
  int s = (2 * channels + 31) / 32;
  if (s % 2 == 0) ++s;
  return 32 * s;
}

template <int NS, int TN, int TK>
struct SpWgradLds {
  static constexpr int PIX = 128;
  static constexpr int SA = sp_row_stride(16 * TN), SB = sp_row_stride(16 * TK);
  static constexpr int PIECE = PIX * (SA + SB);
  static constexpr int STAGE = sp_np(NS) * PIECE;
  static constexpr int RED = 4 * TK * 256 * 4;            // cross-wave reduction, one row of tiles at a time
  static constexpr int BYTES = (STAGE > RED) ? STAGE : RED;
};

template <int NS, int TN, int TK>
__device__ __forceinline__ void wgrad_sp_body(const WgradArgs& p, unsigned char* lds, const int bx, int id) {
  using L = SpWgradLds<NS, TN, TK>;
  constexpr int PIX = L::PIX, SA = L::SA, SB = L::SB, PIECE = L::PIECE;
  constexpr int ROWS = PIX / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nct = p.Cout / (16 * TN), nkt = p.Cin / (16 * TK);
  const int kt = id % nkt;
  id /= nkt;
  const int ct = id % nct;
  const int tap = id / nct;
  const int n0 = ct * 16 * TN, k0 = kt * 16 * TK;
  const int pad = (p.ks - 1) / 2;
  const int kh = tap / p.ks - pad, kw = tap % p.ks - pad;

  const int lo = bx * p.pix_per_block;
  const int hi = min(lo + p.pix_per_block, p.M);
  const int nstages = (hi - lo + PIX - 1) / PIX;
  const int q = tid & 3, r0 = tid >> 2;
  float dyscale, dyinv;                     // fp16x2: the gradient operand is scaled by 2^14 / 2^floor(log2 |max|)
  sp_pow2_scale(p.dymax, dyscale, dyinv);

  const int hw = p.Ho * p.Wo;
  const int b_lo = lo / hw;
  const __amdgpu_buffer_rsrc_t rdy = make_rsrc(p.dy + (size_t)lo * p.lddy, (size_t)max(hi - lo, 0) * p.lddy * 4);
  const __amdgpu_buffer_rsrc_t rx =
      make_rsrc(p.x + (size_t)b_lo * p.Hi * p.Wi * p.ldx, (size_t)(p.B - b_lo) * p.Hi * p.Wi * p.ldx * 4);

  f32x4 ra[ROWS][TN], rb[ROWS][TK];
  auto stage_load = [&](int s) {
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      const int ml = s * PIX + r0 + 64 * i;
      const int m = lo + ml;
      const bool ok = m < hi;
      const unsigned dyo = ok ? ((unsigned)ml * (unsigned)p.lddy + (unsigned)(n0 + 4 * q)) * 4u : HRSEG_BUF_OOB;
#pragma unroll
      for (int j = 0; j < TN; ++j) ra[i][j] = buf_load4(rdy, dyo, 64 * j);
      const int b = fdiv(m, hw, p.rcp_hw);
      const int rem = m - b * hw;
      const int oy = fdiv(rem, p.Wo, p.rcp_w), ox = rem - oy * p.Wo;
      const int iy = oy * p.stride + kh, ix = ox * p.stride + kw;
      const bool okx = ok & (iy >= 0) & (iy < p.Hi) & (ix >= 0) & (ix < p.Wi);
      const unsigned xo =
          okx ? ((unsigned)(((b - b_lo) * p.Hi + iy) * p.Wi + ix) * (unsigned)p.ldx + (unsigned)(k0 + 4 * q)) * 4u
              : HRSEG_BUF_OOB;
#pragma unroll
      for (int j = 0; j < TK; ++j) rb[i][j] = buf_load4(rx, xo, 64 * j);
    }
  };
  auto stage_store = [&]() {
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      const int r = r0 + 64 * i;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        u32x2 pc[sp_np(NS)];
        sp_split4<NS>(ra[i][j], pc, dyscale);
#pragma unroll
        for (int s = 0; s < sp_np(NS); ++s) *reinterpret_cast<u32x2*>(lds + s * PIECE + r * SA + (16 * j + 4 * q) * 2) = pc[s];
      }
#pragma unroll
      for (int j = 0; j < TK; ++j) {
        u32x2 pc[sp_np(NS)];
        sp_split4<NS>(rb[i][j], pc);
#pragma unroll
        for (int s = 0; s < sp_np(NS); ++s)
          *reinterpret_cast<u32x2*>(lds + s * PIECE + PIX * SA + r * SB + (16 * j + 4 * q) * 2) = pc[s];
      }
    }
  };

  f32x4 acc[TN][TK];
#pragma unroll
  for (int n = 0; n < TN; ++n)
#pragma unroll
    for (int k = 0; k < TK; ++k) acc[n][k] = f32x4{0.f, 0.f, 0.f, 0.f};

  // transposed-read addresses: lane 16g+i supplies row (i>>2) of its group's 4-pixel block, columns 4(i&3)..+3
  const int g = lane >> 4, li = lane & 15;
  const int prow = wave * 32 + 4 * g + (li >> 2);
  const int aoff = prow * SA + (li & 3) * 8, boff = PIX * SA + prow * SB + (li & 3) * 8;

  if (nstages > 0) {
    stage_load(0);
    stage_store();
  }
  __syncthreads();
  for (int s = 0; s < nstages; ++s) {
    const bool more = s + 1 < nstages;
    if (more) stage_load(s + 1);
    bf16x8 bfr[TK][sp_np(NS)];
#pragma unroll
    for (int k = 0; k < TK; ++k)
#pragma unroll
      for (int pc = 0; pc < sp_np(NS); ++pc) {
        const s16x4 v0 = sp_tr_read(lds + pc * PIECE + boff + k * 32);
        const s16x4 v1 = sp_tr_read(lds + pc * PIECE + boff + k * 32 + 16 * SB);
        bfr[k][pc] = __builtin_bit_cast(bf16x8, (s16x8){v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]});
      }
#pragma unroll
    for (int n = 0; n < TN; ++n) {
      bf16x8 afr[sp_np(NS)];
#pragma unroll
      for (int pc = 0; pc < sp_np(NS); ++pc) {
        const s16x4 v0 = sp_tr_read(lds + pc * PIECE + aoff + n * 32);
        const s16x4 v1 = sp_tr_read(lds + pc * PIECE + aoff + n * 32 + 16 * SA);
        afr[pc] = __builtin_bit_cast(bf16x8, (s16x8){v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]});
      }
#pragma unroll
      for (int pr = 0; pr < sp_nprod(NS); ++pr)
#pragma unroll
        for (int k = 0; k < TK; ++k) acc[n][k] = sp_mma_p<NS>(pr, afr, bfr[k], acc[n][k]);
    }
    __syncthreads();                       // every wave is done reading before the image is rewritten
    if (more) stage_store();
    __syncthreads();
  }

  // cross-wave reduction, one row of tiles at a time: red[wave][k][reg*64 + lane] (fp32)
  float* red = reinterpret_cast<float*>(lds);
  const int r = tid >> 6, l = tid & 63;
#pragma unroll
  for (int n = 0; n < TN; ++n) {
#pragma unroll
    for (int k = 0; k < TK; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[(wave * TK + k) * 256 + e * 64 + lane] = acc[n][k][e];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TK; ++k) {
      float v = 0.f;
#pragma unroll
      for (int wv = 0; wv < 4; ++wv) v += red[(wv * TK + k) * 256 + tid];
      const int co = n0 + 16 * n + 4 * (l >> 4) + r;  // D row = 4*(lane>>4)+reg
      const int ci = k0 + 16 * k + (l & 15);          // D col = lane&15
      atomicAdd(p.dw + ((size_t)co * p.T + tap) * p.Cin + ci, NS == 4 ? v * dyinv : v);
    }
    __syncthreads();
  }
}

template <int NS, int TN, int TK>
__global__ __launch_bounds__(256) void wgrad_sp_kernel(WgradArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[SpWgradLds<NS, TN, TK>::BYTES];
  const int tiles = gridDim.y, nblk = gridDim.x * gridDim.y;
  const int r = xcd_remap(blockIdx.y * gridDim.x + blockIdx.x, nblk);
  wgrad_sp_body<NS, TN, TK>(p, lds, r / tiles, r % tiles);
}

// --------------------------------------------------------------------------- wide-tile weight gradient
// The tap-per-block body above gives every wave its own 32 pixels of a stage and the WHOLE tile, so the tile is bounded by
// one wave's accumulators (80 x 80) and every operand row is pulled Cin / 80 resp. Cout / 80 times: on the 720 -> 720 layer
// 10 GB through L2 at the ~7.5 TB/s that path delivers = the 1.32 ms the launch takes (MFMA-busy 0.18).  Here the NWR x NWC
// waves of a block share the 32 pixels of a stage and each owns a (16 TN) x (16 TK) part of the block's (16 TN NWR) x (16 TK NWC)
// tile (240 x 144 with 3 x 3 waves of 80 x 48): per pixel 384 operand channels are pulled for 34,560 outputs instead of 160
// for 6,400, no cross-wave reduction, one atomic add per element and block.  Single LDS buffer, the next stage prefetched
// into registers across the MFMAs; 576 threads, 60 KB of LDS, one block per CU.
template <int NS, int TN, int TK, int NWR, int NWC>
struct SpWgradWideLds {
  static constexpr int PIX = 32;
  static constexpr int CA = 16 * TN * NWR, CB = 16 * TK * NWC;        // block tile: output channels x input channels
  static constexpr int SA = sp_row_stride(CA), SB = sp_row_stride(CB);
  static constexpr int PIECE = PIX * (SA + SB);
  static constexpr int BYTES = sp_np(NS) * PIECE;
};

template <int NS, int TN, int TK, int NWR, int NWC>
__device__ __forceinline__ void wgrad_spw_body(const WgradArgs& p, unsigned char* lds, const int bx, int id) {
  using L = SpWgradWideLds<NS, TN, TK, NWR, NWC>;
  constexpr int PIX = L::PIX, SA = L::SA, SB = L::SB, PIECE = L::PIECE, CA = L::CA, CB = L::CB;
  constexpr int NT = 64 * NWR * NWC;
  constexpr int QA = CA / 4, QB = CB / 4;                              // float4 columns of a pixel row
  constexpr int LA = (PIX * QA + NT - 1) / NT, LB = (PIX * QB + NT - 1) / NT;      // loads per thread and stage
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave / NWC, wc = wave % NWC;
  const int nct = p.Cout / CA, nkt = p.Cin / CB;
  const int kt = id % nkt;
  id /= nkt;
  const int ct = id % nct;
  const int tap = id / nct;
  const int n0 = ct * CA, k0 = kt * CB;
  const int pad = (p.ks - 1) / 2;
  const int kh = tap / p.ks - pad, kw = tap % p.ks - pad;
  const int lo = bx * p.pix_per_block;
  const int hi = min(lo + p.pix_per_block, p.M);
  const int nstages = (hi - lo + PIX - 1) / PIX;
  float dyscale, dyinv;
  sp_pow2_scale(p.dymax, dyscale, dyinv);
  const int hw = p.Ho * p.Wo;
  const int b_lo = lo / hw;
  const __amdgpu_buffer_rsrc_t rdy = make_rsrc(p.dy + (size_t)lo * p.lddy, (size_t)max(hi - lo, 0) * p.lddy * 4);
  const __amdgpu_buffer_rsrc_t rx =
      make_rsrc(p.x + (size_t)b_lo * p.Hi * p.Wi * p.ldx, (size_t)(p.B - b_lo) * p.Hi * p.Wi * p.ldx * 4);

  f32x4 ra[LA], rb[LB];
  auto stage_load = [&](int s) {
#pragma unroll
    for (int i = 0; i < LA; ++i) {
      const int u = tid + NT * i, r = u / QA, cq = u - r * QA;
      const int ml = s * PIX + r;
      const bool ok = (u < PIX * QA) & (lo + ml < hi);
      ra[i] = buf_load4(rdy, ok ? ((unsigned)ml * (unsigned)p.lddy + (unsigned)(n0 + 4 * cq)) * 4u : HRSEG_BUF_OOB, 0);
    }
#pragma unroll
    for (int i = 0; i < LB; ++i) {
      const int u = tid + NT * i, r = u / QB, cq = u - r * QB;
      const int m = lo + s * PIX + r;
      const int b = fdiv(m, hw, p.rcp_hw);
      const int rem = m - b * hw;
      const int oy = fdiv(rem, p.Wo, p.rcp_w), ox = rem - oy * p.Wo;
      const int iy = oy * p.stride + kh, ix = ox * p.stride + kw;
      const bool ok = (u < PIX * QB) & (m < hi) & (iy >= 0) & (iy < p.Hi) & (ix >= 0) & (ix < p.Wi);
      rb[i] = buf_load4(rx, ok ? ((unsigned)(((b - b_lo) * p.Hi + iy) * p.Wi + ix) * (unsigned)p.ldx + (unsigned)(k0 + 4 * cq)) * 4u
                               : HRSEG_BUF_OOB, 0);
    }
  };
  auto stage_store = [&]() {
#pragma unroll
    for (int i = 0; i < LA; ++i) {
      const int u = tid + NT * i, r = u / QA, cq = u - r * QA;
      u32x2 pc[sp_np(NS)];
      sp_split4<NS>(ra[i], pc, dyscale);
      if (u < PIX * QA)
#pragma unroll
        for (int q = 0; q < sp_np(NS); ++q) *reinterpret_cast<u32x2*>(lds + q * PIECE + r * SA + cq * 8) = pc[q];
    }
#pragma unroll
    for (int i = 0; i < LB; ++i) {
      const int u = tid + NT * i, r = u / QB, cq = u - r * QB;
      u32x2 pc[sp_np(NS)];
      sp_split4<NS>(rb[i], pc);
      if (u < PIX * QB)
#pragma unroll
        for (int q = 0; q < sp_np(NS); ++q) *reinterpret_cast<u32x2*>(lds + q * PIECE + PIX * SA + r * SB + cq * 8) = pc[q];
    }
  };

  f32x4 acc[TN][TK];
#pragma unroll
  for (int n = 0; n < TN; ++n)
#pragma unroll
    for (int k = 0; k < TK; ++k) acc[n][k] = f32x4{0.f, 0.f, 0.f, 0.f};

  // transposed-read addresses (as in wgrad_sp_body; all waves read the SAME 32 pixels, their own channel columns)
  const int g = lane >> 4, li = lane & 15;
  const int prow = 4 * g + (li >> 2);
  const int aoff = prow * SA + (li & 3) * 8 + wr * TN * 32, boff = PIX * SA + prow * SB + (li & 3) * 8 + wc * TK * 32;

  if (nstages > 0) {
    stage_load(0);
    stage_store();
  }
  __syncthreads();
  for (int s = 0; s < nstages; ++s) {
    const bool more = s + 1 < nstages;
    if (more) stage_load(s + 1);
    bf16x8 afr[TN][sp_np(NS)];
#pragma unroll
    for (int n = 0; n < TN; ++n)
#pragma unroll
      for (int pc = 0; pc < sp_np(NS); ++pc) {
        const s16x4 v0 = sp_tr_read(lds + pc * PIECE + aoff + n * 32);
        const s16x4 v1 = sp_tr_read(lds + pc * PIECE + aoff + n * 32 + 16 * SA);
        afr[n][pc] = __builtin_bit_cast(bf16x8, (s16x8){v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]});
      }
#pragma unroll
    for (int k = 0; k < TK; ++k) {
      bf16x8 bfr[sp_np(NS)];
#pragma unroll
      for (int pc = 0; pc < sp_np(NS); ++pc) {
        const s16x4 v0 = sp_tr_read(lds + pc * PIECE + boff + k * 32);
        const s16x4 v1 = sp_tr_read(lds + pc * PIECE + boff + k * 32 + 16 * SB);
        bfr[pc] = __builtin_bit_cast(bf16x8, (s16x8){v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]});
      }
#pragma unroll
      for (int pr = 0; pr < sp_nprod(NS); ++pr)
#pragma unroll
        for (int n = 0; n < TN; ++n) acc[n][k] = sp_mma_p<NS>(pr, afr[n], bfr, acc[n][k]);
    }
    __syncthreads();                       // every wave is done reading before the image is rewritten
    if (more) stage_store();
    __syncthreads();
  }

#pragma unroll
  for (int n = 0; n < TN; ++n)
#pragma unroll
    for (int k = 0; k < TK; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int co = n0 + (wr * TN + n) * 16 + 4 * g + e;       // D row = 4*(lane>>4)+reg
        const int ci = k0 + (wc * TK + k) * 16 + li;              // D col = lane&15
        atomicAdd(p.dw + ((size_t)co * p.T + tap) * p.Cin + ci, NS == 4 ? acc[n][k][e] * dyinv : acc[n][k][e]);
      }
}

template <int NS, int TN, int TK, int NWR, int NWC>
__global__ __launch_bounds__(64 * NWR * NWC) void wgrad_spw_kernel(WgradArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[SpWgradWideLds<NS, TN, TK, NWR, NWC>::BYTES];
  const int tiles = gridDim.y, nblk = gridDim.x * gridDim.y;
  const int r = xcd_remap(blockIdx.y * gridDim.x + blockIdx.x, nblk);
  wgrad_spw_body<NS, TN, TK, NWR, NWC>(p, lds, r / tiles, r % tiles);
}

// several problems in one launch (the fuse layers' 1x1 / stride-2 weight gradients of an HRNet module): blocks
// [blk_end[g-1], blk_end[g]) belong to problem g, each with its own pixel ranges x (tap, tile) blocks
template <int NS, int TN, int TK>
__global__ __launch_bounds__(256) void wgrad_sp_group_kernel(WgradGroup grp) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[SpWgradLds<NS, TN, TK>::BYTES];
  int g = 0;
  while (g + 1 < grp.n && (int)blockIdx.x >= grp.blk_end[g]) ++g;
  const int lo = g ? grp.blk_end[g - 1] : 0;
  const int nblk = grp.blk_end[g] - lo;
  const int tiles = nblk / grp.gx[g];
  const int r = xcd_remap(blockIdx.x - lo, nblk);
  wgrad_sp_body<NS, TN, TK>(grp.a[g], lds, r / tiles, r % tiles);
}

// --------------------------------------------------------------------------- weight gradient, 3x3 stride 1: all nine taps per block
// The tap-per-block weight gradient above pulls dy and x through L2 nine times and splits every element nine
// times.  Here a block owns a (16*TNK couts) x (16*TNK cins) tile of dW for ALL nine taps and walks a chunk of
// 4 x 16 pixel tiles: per tile it stages the dy tile (64 pixels) and the (4+2) x 18 x patch ONCE (split on the
// fly, bf16 pieces, [pixel][channel] images) and its three waves -- wave = kernel row kh -- read transposed
// fragments for their three taps kw from the same patch at shifted pixel positions.  The block keeps its
// 3 x TNK x TNK accumulator tiles per wave in registers over the whole chunk and writes them with PLAIN stores
// into its own slab of a workspace [chunk][Cout][9][Cin]; wgrad9_reduce_kernel then adds the chunks to dW in
// index order: no atomics, no cross-wave reduction, and the gradient is bit-reproducible run to run.
template <int NS, int TNK>
struct SpWgrad9Lds {
  static constexpr int S = sp_row_stride(16 * TNK);     // bytes per pixel row (both images)
  static constexpr int DYPIX = 64, XPIX = 6 * 18;
  static constexpr int PIECE = (DYPIX + XPIX) * S;
  static constexpr int BYTES = sp_np(NS) * PIECE;
};

template <int NS, int TNK>
__device__ __forceinline__ void wgrad9_sp_body(const Wgrad9Args& p, unsigned char* lds, const int pair, const int chunk) {
  using L = SpWgrad9Lds<NS, TNK>;
  constexpr int S = L::S, PIECE = L::PIECE, XBASE = L::DYPIX * S;
  constexpr int GPP = TNK * 4;                               // 16-byte granules per pixel
  // a round of the block's 192 threads stages PR whole pixels (thread -> pixel tid / GPP of the round, granule
  // tid % GPP of the pixel): the dy tile takes 64 / PR rounds -- one tile row each when PR = 16 -- and the x patch
  // the rest; no division by a runtime value and one small multiply per granule (a wave issues an instruction every
  // four cycles at best, and with 1.5 waves per SIMD the staging arithmetic is paid in MFMA time)
  constexpr int NT = 192, PR = NT / GPP;
  constexpr int DY_LOADS = (L::DYPIX + PR - 1) / PR, X_LOADS = (L::XPIX + PR - 1) / PR, LOADS = DY_LOADS + X_LOADS;
  const int tid = threadIdx.x, lane = tid & 63, kh = tid >> 6;     // wave = kernel row
  const int g = lane >> 4, li = lane & 15;
  const int nkt = p.Cin / (16 * TNK);
  const int ct = pair / nkt, kt = pair - ct * nkt;
  const int n0 = ct * 16 * TNK, k0 = kt * 16 * TNK;
  const int t_lo = chunk * p.per, t_hi = min(t_lo + p.per, p.ntiles);
  float dyscale, dyinv;                     // fp16x2: the gradient operand is scaled by 2^14 / 2^floor(log2 |max|)
  sp_pow2_scale(p.dymax, dyscale, dyinv);

  f32x4 rg[LOADS];
  const int pix0 = tid / GPP, gq = tid - pix0 * GPP;
  const bool swork = pix0 < PR;                                // (TNK = 3: all 192 threads; TNK = 4: 12 x 16)
  // What a thread's granules are does not depend on the tile: their byte offsets from the tile origin (dy) / the patch origin
  // (x: row y0-1, column x0-1) and their (row, column) there are computed once per block.  A tile that lies inside the image
  // with its halo loads them with these as the vector offset and the tile origin as the SCALAR offset -- no vector
  // instruction per granule; a border tile pays two range tests.  (Per tile this was three integer divisions and, per
  // granule, two quarter-rate 32-bit multiplies: with 1.5 waves per SIMD all of it is paid in MFMA time.)
  unsigned g_rel[LOADS];
  int g_yx[LOADS];                                             // (row << 8) | column; a row no image reaches where the granule does not exist
#pragma unroll
  for (int i = 0; i < LOADS; ++i) {
    if (i < DY_LOADS) {
      const int pix = pix0 + PR * i;
      const bool ex = swork & (pix < L::DYPIX);
      g_rel[i] = ex ? ((unsigned)((pix >> 4) * p.W + (pix & 15)) * (unsigned)p.lddy + (unsigned)(n0 + 4 * gq)) * 4u : HRSEG_BUF_OOB;
      g_yx[i] = ex ? ((pix >> 4) << 8) | (pix & 15) : 0x400000;
    } else {
      const int pix = pix0 + PR * (i - DY_LOADS);
      const int py = (pix * 3641) >> 16, px = pix - py * 18;         // pix / 18
      const bool ex = swork & (pix < L::XPIX);
      g_rel[i] = ex ? ((unsigned)(py * p.W + px) * (unsigned)p.ldx + (unsigned)(k0 + 4 * gq)) * 4u : HRSEG_BUF_OOB;
      g_yx[i] = ex ? (py << 8) | px : 0x400000;
    }
  }
  // tile cursor of the NEXT load (tiles walk columns, rows, images): one division per block
  int c_tx = t_lo % p.tiles_x, c_ty = (t_lo / p.tiles_x) % p.tiles_y, c_b = (t_lo / p.tiles_x) / p.tiles_y;
  c_tx = __builtin_amdgcn_readfirstlane(c_tx); c_ty = __builtin_amdgcn_readfirstlane(c_ty); c_b = __builtin_amdgcn_readfirstlane(c_b);
  const unsigned lddy4 = (unsigned)p.lddy * 4u, ldx4 = (unsigned)p.ldx * 4u;
  auto tile_load = [&]() {
    const int y0 = c_ty * 4, x0 = c_tx * 16;
    const __amdgpu_buffer_rsrc_t rdy = make_rsrc(p.dy + (size_t)c_b * p.H * p.W * p.lddy, (size_t)p.H * p.W * p.lddy * 4);
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x + (size_t)c_b * p.H * p.W * p.ldx, (size_t)p.H * p.W * p.ldx * 4);
    const unsigned dyb = (unsigned)(y0 * p.W + x0) * lddy4;
    const unsigned xb = (unsigned)((y0 - 1) * p.W + x0 - 1) * ldx4;          // (mod 2^32 on a border tile: only added to offsets that exist)
    const bool dy_full = (y0 + 4 <= p.H) & (x0 + 16 <= p.W);
    const bool x_full = (y0 >= 1) & (x0 >= 1) & (y0 + 5 <= p.H) & (x0 + 17 <= p.W);
    if (dy_full) {
#pragma unroll
      for (int i = 0; i < DY_LOADS; ++i) rg[i] = buf_load4(rdy, g_rel[i], (int)dyb);
    } else {
#pragma unroll
      for (int i = 0; i < DY_LOADS; ++i) {
        const bool ok = (y0 + (g_yx[i] >> 8) < p.H) & (x0 + (g_yx[i] & 255) < p.W);
        rg[i] = buf_load4(rdy, ok ? g_rel[i] + dyb : HRSEG_BUF_OOB, 0);
      }
    }
    if (x_full) {
#pragma unroll
      for (int i = DY_LOADS; i < LOADS; ++i) rg[i] = buf_load4(rx, g_rel[i], (int)xb);
    } else {
#pragma unroll
      for (int i = DY_LOADS; i < LOADS; ++i) {
        const bool ok = ((unsigned)(y0 - 1 + (g_yx[i] >> 8)) < (unsigned)p.H) & ((unsigned)(x0 - 1 + (g_yx[i] & 255)) < (unsigned)p.W);
        rg[i] = buf_load4(rx, ok ? g_rel[i] + xb : HRSEG_BUF_OOB, 0);
      }
    }
    if (++c_tx == p.tiles_x) {
      c_tx = 0;
      if (++c_ty == p.tiles_y) { c_ty = 0; ++c_b; }
    }
  };
  auto tile_store = [&]() {
    // both images are [pixel][S bytes], the x patch behind the dy tile
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      u32x2 pc[sp_np(NS)];
      if (i >= DY_LOADS && (p.x_presplit | p.exp_nosplit)) {      // x stored pre-split (hrseg_conv_shape_t.x_split): the 16 bytes ARE {hi01, hi23, lo01, lo23}
        // (exp_nosplit: the same copy on fp32 data, wrong values on purpose: the ceiling measurement of tools/)
        const u32x4 raw = __builtin_bit_cast(u32x4, rg[i]);
#pragma unroll
        for (int s = 0; s < sp_np(NS); ++s) pc[s] = u32x2{raw[(2 * s) & 3], raw[(2 * s + 1) & 3]};
      } else {
        sp_split4<NS>(rg[i], pc, i < DY_LOADS ? dyscale : 1.f);
      }
      const int pix = (i < DY_LOADS) ? pix0 + PR * i : L::DYPIX + pix0 + PR * (i - DY_LOADS);
      const int o = pix * S + gq * 8;
      if (swork && (i < DY_LOADS ? pix < L::DYPIX : pix < L::DYPIX + L::XPIX)) {
#pragma unroll
        for (int s = 0; s < sp_np(NS); ++s) *reinterpret_cast<u32x2*>(lds + s * PIECE + o) = pc[s];
      }
    }
  };

  f32x4 acc[3][TNK][TNK];
#pragma unroll
  for (int w = 0; w < 3; ++w)
#pragma unroll
    for (int n = 0; n < TNK; ++n)
#pragma unroll
      for (int k = 0; k < TNK; ++k) acc[w][n][k] = f32x4{0.f, 0.f, 0.f, 0.f};

  // transposed-read lane offsets: lane 16g+i supplies row (i>>2) of a 4-pixel block, columns 4(i&3)..+3
  const int lrow = li >> 2, lcol = (li & 3) * 8;
  const int dy_lane = (4 * g + lrow) * S + lcol;                              // + (2ks+h)*16*S + n*32
  const int x_lane = XBASE + (kh * 18 + 4 * g + lrow) * S + lcol;             // + ((2ks+h)*18 + kw)*S + k*32

  if (t_lo < t_hi) tile_load();
  for (int t = t_lo; t < t_hi; ++t) {
    __syncthreads();                         // every wave is done with the previous tile's images
    tile_store();
    if (t + 1 < t_hi) tile_load();           // in flight behind this tile's MFMAs
    __syncthreads();
    // Six groups (pixel half ks, kernel column kw) of TNK x TNK tiles.  Inside a group the products go output-channel
    // block k outermost, so the x fragments of block k are dead after its TNK * products MFMAs and the reads of the
    // NEXT group's block k can be issued into the same registers right there, behind the MFMAs still to come (pinned
    // with sched_barrier: left alone the compiler bursts a group's reads in front of its MFMAs and every group starts
    // with an exposed LDS round trip).  Only the dy fragments of the second pixel half are read in the open.
    bf16x8 afr[TNK][sp_np(NS)], bfr[TNK][sp_np(NS)];
    auto read_a = [&](int ks) {
#pragma unroll
      for (int n = 0; n < TNK; ++n)
#pragma unroll
        for (int pc = 0; pc < sp_np(NS); ++pc) {
          const s16x4 v0 = sp_tr_read(lds + pc * PIECE + dy_lane + (2 * ks) * 16 * S + n * 32);
          const s16x4 v1 = sp_tr_read(lds + pc * PIECE + dy_lane + (2 * ks + 1) * 16 * S + n * 32);
          afr[n][pc] = __builtin_bit_cast(bf16x8, (s16x8){v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]});
        }
    };
    auto read_b = [&](int grp, int k) {
      const int ks = grp / 3, kw = grp % 3;
#pragma unroll
      for (int pc = 0; pc < sp_np(NS); ++pc) {
        const s16x4 v0 = sp_tr_read(lds + pc * PIECE + x_lane + ((2 * ks) * 18 + kw) * S + k * 32);
        const s16x4 v1 = sp_tr_read(lds + pc * PIECE + x_lane + ((2 * ks + 1) * 18 + kw) * S + k * 32);
        bfr[k][pc] = __builtin_bit_cast(bf16x8, (s16x8){v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]});
      }
    };
    read_a(0);
#pragma unroll
    for (int k = 0; k < TNK; ++k) read_b(0, k);
#pragma unroll
    for (int grp = 0; grp < 6; ++grp) {
      const int kw = grp % 3;
      if (grp == 3) read_a(1);
#pragma unroll
      for (int k = 0; k < TNK; ++k) {
#pragma unroll
        for (int pr = 0; pr < sp_nprod(NS); ++pr)
#pragma unroll
          for (int n = 0; n < TNK; ++n) acc[kw][n][k] = sp_mma_p<NS>(pr, afr[n], bfr[k], acc[kw][n][k]);
        __builtin_amdgcn_sched_barrier(0);
        if (grp + 1 < 6) read_b(grp + 1, k);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  // this block's slab of the workspace: plain stores, every element written by exactly one lane
  float* out = p.ws + (size_t)chunk * p.Cout * 9 * p.Cin;
  const int row9 = 9 * p.Cin;
  const int obase = ((n0 + 4 * g) * 9 + kh * 3) * p.Cin + k0 + li;     // D row = 4*(lane>>4)+reg, D col = lane&15
#pragma unroll
  for (int kw = 0; kw < 3; ++kw)
#pragma unroll
    for (int n = 0; n < TNK; ++n)
#pragma unroll
      for (int k = 0; k < TNK; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          out[obase + (16 * n + e) * row9 + kw * p.Cin + 16 * k] = NS == 4 ? acc[kw][n][k][e] * dyinv : acc[kw][n][k][e];
}

template <int NS, int TNK>
__device__ __forceinline__ void wgrad9_sp_group_entry(const Wgrad9Group& grp, unsigned char* lds) {
  const int bid = (int)blockIdx.x;
  int gi = 0;
  while (gi + 1 < grp.n && bid >= grp.blk_end[gi]) ++gi;
  const int local = bid - (gi ? grp.blk_end[gi - 1] : 0);
  const Wgrad9Args& p = grp.a[gi];
  const int npairs = (p.Cout / (16 * TNK)) * (p.Cin / (16 * TNK));
  wgrad9_sp_body<NS, TNK>(p, lds, local % npairs, local / npairs);     // the tile pairs of one chunk are neighbours: same pixels
}
// 48-channel tiles: capped at 256 registers so that two blocks (six waves) share a CU
template <int NS>
__global__ __launch_bounds__(192) __attribute__((amdgpu_waves_per_eu(2, 2))) void wgrad9_sp_group_kernel3(Wgrad9Group grp) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[SpWgrad9Lds<NS, 3>::BYTES];
  wgrad9_sp_group_entry<NS, 3>(grp, lds);
}
// 64-channel tiles: 3 x 16 accumulator tiles per wave, one block per CU
template <int NS>
__global__ __launch_bounds__(192) void wgrad9_sp_group_kernel4(Wgrad9Group grp) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[SpWgrad9Lds<NS, 4>::BYTES];
  wgrad9_sp_group_entry<NS, 4>(grp, lds);
}

__global__ __launch_bounds__(256) void wgrad9_reduce_kernel(Wgrad9Reduce r) {
  // block = 32 consecutive float4 x 8 chunk groups (group j sums chunks j, j+8, ... in order); the eight partial
  // sums meet in LDS and are added in a fixed tree order: the same bits every run
  __shared__ f32x4 part[8][32];
  int gi = 0;
  while (gi + 1 < r.n && (int)blockIdx.x >= r.blk_end[gi]) ++gi;
  const int lo = gi ? r.blk_end[gi - 1] : 0;
  const long n4 = r.n4[gi];
  const f32x4* ws = reinterpret_cast<const f32x4*>(r.ws[gi]);
  f32x4* dw = reinterpret_cast<f32x4*>(r.dw[gi]);
  const int nch = r.nchunks[gi];
  const int e = threadIdx.x & 31, j = threadIdx.x >> 5;
  for (long i0 = (long)(blockIdx.x - lo) * 32; i0 < n4; i0 += (long)(r.blk_end[gi] - lo) * 32) {
    const long i = i0 + e;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (i < n4)
      for (int c = j; c < nch; c += 8) s += ws[(size_t)c * n4 + i];
    part[j][e] = s;
    __syncthreads();
    if (j == 0 && i < n4)
      dw[i] += ((part[0][e] + part[1][e]) + (part[2][e] + part[3][e])) + ((part[4][e] + part[5][e]) + (part[6][e] + part[7][e]));
    __syncthreads();
  }
}

// --------------------------------------------------------------------------- launchers
template <int NS>
static int launch_wgrad_sp(const WgradArgs& a, int tn, int tk, int gx, int tiles, hipStream_t st) {
#define WS(TN_, TK_) if (tn == TN_ && tk == TK_) { hipLaunchKernelGGL((wgrad_sp_kernel<NS, TN_, TK_>), dim3(gx, tiles), dim3(256), 0, st, a); return 0; }
  WS(1, 1) WS(1, 2) WS(1, 3) WS(1, 4) WS(2, 1) WS(2, 2) WS(2, 3) WS(2, 4)
  WS(3, 1) WS(3, 2) WS(3, 3) WS(3, 4) WS(4, 1) WS(4, 2) WS(4, 3) WS(4, 4)
  if constexpr (NS == 4) { WS(5, 5) }       // 80 x 80 tile (80 KB of LDS, one block per CU): the 720-channel layer
#undef WS
  return HRSEG_ERR_UNSUPPORTED;
}
int launch_wgrad_sp_kernel(int ns, const WgradArgs& a, int tn, int tk, int gx, int tiles, hipStream_t st) {
  return ns == 4 ? launch_wgrad_sp<4>(a, tn, tk, gx, tiles, st) : ns == 3 ? launch_wgrad_sp<3>(a, tn, tk, gx, tiles, st)
       : ns == 2 ? launch_wgrad_sp<2>(a, tn, tk, gx, tiles, st) : launch_wgrad_sp<1>(a, tn, tk, gx, tiles, st);
}
// fp16x2, 240 x 144 block tiles (nwc = 3: 3 x 3 waves) or 240 x 48 (nwc = 1: 3 waves, the layers of 48 input channels)
int launch_wgrad_spw_kernel(const WgradArgs& a, int nwc, int gx, int tiles, hipStream_t st) {
  if (nwc == 3) hipLaunchKernelGGL((wgrad_spw_kernel<4, 5, 3, 3, 3>), dim3(gx, tiles), dim3(576), 0, st, a);
  else hipLaunchKernelGGL((wgrad_spw_kernel<4, 5, 3, 3, 1>), dim3(gx, tiles), dim3(192), 0, st, a);
  return 0;
}
int launch_wgrad_group_sp(const WgradGroup& g, int tn, int tk, int nblocks, hipStream_t st) {      // fp16x2 only
#define WGS(TN_, TK_) if (tn == TN_ && tk == TK_) { hipLaunchKernelGGL((wgrad_sp_group_kernel<4, TN_, TK_>), dim3(nblocks), dim3(256), 0, st, g); return 0; }
  WGS(3, 3) WGS(3, 4) WGS(4, 3) WGS(4, 4)
#undef WGS
  return 1;
}
int launch_wgrad9_kernels(int ns, int tnk, const Wgrad9Group& g, int nblocks, const Wgrad9Reduce& r, int rblocks, hipStream_t st) {
#define W9(NS_) if (ns == NS_) { \
    if (tnk == 3) hipLaunchKernelGGL((wgrad9_sp_group_kernel3<NS_>), dim3(nblocks), dim3(192), 0, st, g); \
    else hipLaunchKernelGGL((wgrad9_sp_group_kernel4<NS_>), dim3(nblocks), dim3(192), 0, st, g); }
  W9(1) W9(2) W9(3) W9(4)
#undef W9
  HRSEG_LAUNCH_CHECK("wgrad9");
  hipLaunchKernelGGL(wgrad9_reduce_kernel, dim3(rblocks), dim3(256), 0, st, r);
  HRSEG_LAUNCH_CHECK("wgrad9_reduce");
  return 0;
}
