// Split-precision implicit GEMM, im2col body (igemm_sp_body) and its plain and grouped kernels: used by conv_sp_im2col.hip and
// conv_sp_pgroup.hip.  Arithmetic (piece schemes, split, products): sp_arith.h.
//
// Layout of one block (256 threads, 4 waves): GEMM rows = 64*WTM output pixels, each wave owns 16*WTM of
// them; columns = 16*WTN output channels.  The PIXEL operand never touches LDS: lane (r = l&15, g = l>>4)
// loads, for its own pixel row r of every 16-row tile, channels 4g..4g+3 of the slab's two 16-channel units
// (two 16-byte buffer loads), splits them in registers and has the MFMA B fragment (k = 8g..8g+7) in place.
// Only the WEIGHT slab goes through LDS (all four waves read every weight fragment): [piece][row][64 B],
// XOR-swizzled 16-byte slots, double buffered, one barrier per slab.  The k index inside a slab is
// permuted the same way on both operands: k = 8g+j  <->  unit j>>2, channel 4g + (j&3).
#pragma once
#include "conv_common.h"
#include "sp_arith.h"

template <int NS, int WTN>
struct SpLds {
  static constexpr int BN = 16 * WTN;
  static constexpr int PIECE = BN * 64;          // bytes: one slab of one piece, [BN rows][32 bf16]
  static constexpr int STAGE = sp_np(NS) * PIECE;       // one buffer
  static constexpr int BYTES = 2 * STAGE;        // double buffered
};

#define SP_DEPTH 3        // slabs of global-load look-ahead in igemm_sp_body
// One output tile of one convolution.  `ks_idx / ks_n`: split-K slice of the slab list (partial sums are
// added with fp32 atomics, as in igemm_body).
template <int NS, int WTM, int WTN>
__device__ __forceinline__ void igemm_sp_body(const IgemmArgs& p, unsigned char* lds, const int bid, const int nblk,
                                              const int ks_idx, const int ks_n) {
  constexpr int BM = 64 * WTM, BN = 16 * WTN;
  constexpr int PIECE = SpLds<NS, WTN>::PIECE, STAGE = SpLds<NS, WTN>::STAGE;
  constexpr int WG = BN * 8;                       // 16-byte weight granules per slab
  constexpr int W_LOADS = (WG + 255) / 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int ntn = p.N / BN;
  const int wg = xcd_remap(bid, nblk);
  const int m0 = (wg / ntn) * BM, n0 = (wg % ntn) * BN;

  float xscale, xinv;                       // fp16x2: power-of-two scale of the pixel operand (a gradient: from its |max|)
  sp_pow2_scale(p.xmax, xscale, xinv);
  const float oscale = xinv * p.wscale_inv;

  // reduction index: units of 16 channels, u = tap * kch + chunk; a slab = units 2s, 2s+1
  const int kch = p.K >> 4;
  const int nunits = p.ntaps * kch;
  const int nslabs_all = (nunits + 1) >> 1;
  const int per = (nslabs_all + ks_n - 1) / ks_n;
  const int s_lo = ks_idx * per;
  const int s_hi = min(s_lo + per, nslabs_all);
  const int nslabs = s_hi - s_lo;

  // Input descriptor: based at the first image this tile touches, moved back by the most negative tap
  // offset, so that every lane offset and every per-tap scalar offset is non-negative.  Memory in front of
  // the tensor is never read: taps outside the image get the out-of-range offset (zero fill).
  const int hw = p.Ho * p.Wo;
  const int b0 = m0 / hw;
  const long tap0 = (long)p.oy_min * p.Wi + p.ox_min;          // <= 0
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x + ((long)b0 * p.Hi * p.Wi + tap0) * p.ldx,
                                              (size_t)((long)(p.B - b0) * p.Hi * p.Wi - tap0) * p.ldx * 4);
  const __amdgpu_buffer_rsrc_t rw = make_rsrc(p.w, (size_t)p.N * p.T * p.K * 4);

  // this lane's pixel rows: byte offset of (pixel at tap offset 0, channel 4g) and the taps that fall outside
  unsigned voff[WTM];
  int inval[WTM];
#pragma unroll
  for (int m = 0; m < WTM; ++m) {
    const int row = m0 + wave * 16 * WTM + 16 * m + r16;
    if (row < p.M) {
      const int b = fdiv(row, hw, p.rcp_hw);
      const int rem = row - b * hw;
      const int oy = fdiv(rem, p.Wo, p.rcp_w), ox = rem - oy * p.Wo;
      const int iy0 = oy * p.sy, ix0 = ox * p.sx;
      voff[m] = ((unsigned)((b - b0) * p.Hi * p.Wi + iy0 * p.Wi + ix0) * (unsigned)p.ldx + 4u * g) * 4u;
      int bad = 0;
      for (int t = 0; t < p.ntaps; ++t) {
        const int iy = iy0 + (int)((p.offy_pk >> (4 * t)) & 15) - 8, ix = ix0 + (int)((p.offx_pk >> (4 * t)) & 15) - 8;
        bad |= ((iy < 0) | (iy >= p.Hi) | (ix < 0) | (ix >= p.Wi)) ? (1 << t) : 0;
      }
      inval[m] = bad;
    } else {
      voff[m] = 0;
      inval[m] = -1;
    }
  }

  // weight granules of this thread: granule f = (row n = f>>3, unit (f>>2)&1, 4-channel group f&3)
  unsigned wbase[W_LOADS];
  int wunit[W_LOADS], wst[W_LOADS];
#pragma unroll
  for (int i = 0; i < W_LOADS; ++i) {
    const int f = tid + 256 * i;
    const int n = f >> 3, unit = (f >> 2) & 1, gq = f & 3;
    wbase[i] = (f < WG) ? ((unsigned)(n0 + n) * (unsigned)(p.T * p.K) + 4u * gq) * 4u : HRSEG_BUF_OOB;
    wunit[i] = unit;
    wst[i] = n * 64 + lds_slot(n, gq) * 16 + unit * 8;
  }

  // running unit counters (scalar): tap and chunk of the next slab's two units.  Loads run SP_DEPTH slabs
  // ahead of their use in a ring of register sets: a slab of this body is 6-36 MFMAs per wave (0.1-0.3 us), an
  // L2 round trip under load is several times that, and with one or two blocks per CU nothing else hides it
  // (measured: 1.2 us per slab with one slab of look-ahead on the low-resolution branches).  Every load is
  // issued unconditionally -- past the end of the slice with out-of-range offsets (zero fill, no traffic) -- so
  // the vmcnt bookkeeping stays exact and a slab waits for its own loads only.
  constexpr int D = SP_DEPTH;
  int u_next = 2 * s_lo;
  const int u_end = min(nunits, 2 * s_hi);
  // (tap, chunk) of unit u_next, stepped unit by unit: ONE division per block (a division per unit is ~25 vector instructions
  // twice per slab, in a body whose slab is 6-36 MFMAs)
  int u_t = __builtin_amdgcn_readfirstlane(u_next / kch), u_c = u_next - u_t * kch;
  f32x4 ra[D][WTM][2], rwt[D][W_LOADS];
  auto issue_loads = [&](f32x4 (&ra)[WTM][2], f32x4 (&rwt)[W_LOADS]) {
    unsigned soff[2], wsoff[2];
    int tapbit[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int u = u_next + h;
      const bool live = u < u_end;
      const int t = live ? u_t : 0;
      const int c = live ? u_c : 0;
      if (++u_c == kch) { u_c = 0; ++u_t; }
      const int dy = (int)((p.offy_pk >> (4 * t)) & 15) - 8 - p.oy_min, dx = (int)((p.offx_pk >> (4 * t)) & 15) - 8 - p.ox_min;
      soff[h] = (unsigned)((dy * p.Wi + dx) * p.ldx + 16 * c) * 4u;
      wsoff[h] = live ? (unsigned)((int)((p.wtap_pk >> (4 * t)) & 15) * p.K + 16 * c) * 4u : HRSEG_BUF_OOB;
      tapbit[h] = live ? t : 31;          // bit 31 of inval is set only for rows past M; dead unit: forced below
      if (!live) soff[h] = 0;
    }
    const bool live0 = u_next < u_end, live1 = u_next + 1 < u_end;
#pragma unroll
    for (int m = 0; m < WTM; ++m) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        // -1 (out of range: zero fill) when the tap is outside the image for this row or the unit is dead
        const int oob = __builtin_amdgcn_sbfe(inval[m], tapbit[h], 1) | ((h == 1 ? !live1 : !live0) ? -1 : 0);
        ra[m][h] = buf_load4(rx, voff[m] | (unsigned)oob, (int)soff[h]);
      }
    }
#pragma unroll
    for (int i = 0; i < W_LOADS; ++i) {
      const unsigned so = wunit[i] ? wsoff[1] : wsoff[0];
      const unsigned off = (wbase[i] == HRSEG_BUF_OOB || so == HRSEG_BUF_OOB) ? HRSEG_BUF_OOB : wbase[i] + so;
      rwt[i] = buf_load4(rw, off, 0);
    }
    u_next += 2;
  };

  bf16x8 xf[WTM][sp_np(NS)];
  auto split_store = [&](int buf, const f32x4 (&ra)[WTM][2], const f32x4 (&rwt)[W_LOADS]) {
    unsigned char* base = lds + buf * STAGE;
#pragma unroll
    for (int i = 0; i < W_LOADS; ++i) {
      u32x2 pc[sp_np(NS)];
      sp_split4<NS>(rwt[i], pc, p.wscale);
      if (tid + 256 * i < WG) {
#pragma unroll
        for (int s = 0; s < sp_np(NS); ++s) *reinterpret_cast<u32x2*>(base + s * PIECE + wst[i]) = pc[s];
      }
    }
#pragma unroll
    for (int m = 0; m < WTM; ++m) sp_split8<NS>(ra[m][0], ra[m][1], xf[m], xscale);
  };

  f32x4 acc[WTN][WTM];
#pragma unroll
  for (int n = 0; n < WTN; ++n)
#pragma unroll
    for (int m = 0; m < WTM; ++m) acc[n][m] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int foff = r16 * 64 + lds_slot(r16, g) * 16;       // weight fragment of this lane inside a 16-row tile

  // slab s lives in register set s % D; the slab count is padded to a multiple of D (dead slabs are zeros)
#pragma unroll
  for (int d = 0; d < D; ++d) issue_loads(ra[d], rwt[d]);
  split_store(0, ra[0], rwt[0]);
  __syncthreads();
  for (int s0 = 0; s0 < nslabs; s0 += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int s = s0 + d;
      issue_loads(ra[d], rwt[d]);                        // slab s + D; set d held slab s, consumed a slab ago
      const unsigned char* base = lds + (s & 1) * STAGE;
#pragma unroll
      for (int n = 0; n < WTN; ++n) {
        bf16x8 wf[sp_np(NS)];
#pragma unroll
        for (int q = 0; q < sp_np(NS); ++q) wf[q] = *reinterpret_cast<const bf16x8*>(base + q * PIECE + n * 1024 + foff);
#pragma unroll
        for (int pr = 0; pr < sp_nprod(NS); ++pr)
#pragma unroll
          for (int m = 0; m < WTM; ++m) acc[n][m] = sp_mma_p<NS>(pr, wf, xf[m], acc[n][m]);
      }
      split_store((s + 1) & 1, ra[(d + 1) % D], rwt[(d + 1) % D]);      // slab s + 1
      __syncthreads();
    }
  }

  // epilogue: lane holds channels n0+16n+4g..+3 of pixel row r16 of every tile
  // (all reads -- bias, the values an accumulating launch adds to -- before the first store: a read behind every
  // store is a memory round trip each, see igemm_patch_ws_body)
  const bool split = ks_n > 1;
  float* yrows[WTM];
  f32x4 add[WTM][WTN];
#pragma unroll
  for (int n = 0; n < WTN; ++n) {
    f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
    if (p.bias && ks_idx == 0) bv = *reinterpret_cast<const f32x4*>(p.bias + n0 + 16 * n + 4 * g);
#pragma unroll
    for (int m = 0; m < WTM; ++m) add[m][n] = bv;
  }
#pragma unroll
  for (int m = 0; m < WTM; ++m) {
    const int row = m0 + wave * 16 * WTM + 16 * m + r16;
    yrows[m] = nullptr;
    if (row >= p.M) continue;
    size_t pix = row;
    if (!p.direct_out) {
      const int b = fdiv(row, hw, p.rcp_hw);
      const int rem = row - b * hw;
      const int oy = fdiv(rem, p.Wo, p.rcp_w), ox = rem - oy * p.Wo;
      pix = (size_t)(b * p.Hy + oy * p.oys + p.oy0) * p.Wy + ox * p.oxs + p.ox0;
    }
    yrows[m] = p.y + pix * p.ldy;
    if (p.accumulate && !split) {
#pragma unroll
      for (int n = 0; n < WTN; ++n) add[m][n] += *reinterpret_cast<const f32x4*>(yrows[m] + n0 + 16 * n + 4 * g);
    }
    if (p.res && !split) {
#pragma unroll
      for (int n = 0; n < WTN; ++n) add[m][n] += *reinterpret_cast<const f32x4*>(p.res + pix * p.ldr + n0 + 16 * n + 4 * g);
    }
  }
#pragma unroll
  for (int m = 0; m < WTM; ++m) {
    float* yrow = yrows[m];
    if (!yrow) continue;
#pragma unroll
    for (int n = 0; n < WTN; ++n) {
      const int ch = n0 + 16 * n + 4 * g;
      f32x4 v = acc[n][m];
      if (NS == 4) v *= oscale;
      v += add[m][n];
      if (split) {
#pragma unroll
        for (int e = 0; e < 4; ++e) atomicAdd(yrow + ch + e, v[e]);
      } else {
        if (p.relu) v = relu_nan(v);
        *reinterpret_cast<f32x4*>(yrow + ch) = v;
      }
    }
  }
}

template <int NS, int WTM, int WTN>
__global__ __launch_bounds__(256) void igemm_sp_kernel(IgemmArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[SpLds<NS, WTN>::BYTES];
  igemm_sp_body<NS, WTM, WTN>(p, lds, blockIdx.x, gridDim.x, blockIdx.y, gridDim.y);
}

// grouped form: see igemm_group_kernel
template <int NS, int WTM, int WTN, bool FULL3X3>
__global__ __launch_bounds__(256) void igemm_sp_group_kernel(IgemmGroup grp) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[SpLds<NS, WTN>::BYTES];
  int gi = 0;
  while (gi + 1 < grp.n && (int)blockIdx.x >= grp.blk_end[gi]) ++gi;
  const int local = blockIdx.x - (gi ? grp.blk_end[gi - 1] : 0);
  const int tiles = grp.tiles[gi];
  igemm_sp_body<NS, WTM, WTN>(grp.a[gi], lds, local % tiles, tiles, local / tiles, grp.ksplit[gi]);
}
