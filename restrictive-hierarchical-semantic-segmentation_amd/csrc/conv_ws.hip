// Wave-specialised fp16x2 / bf16 halo-patch kernels (3x3 stride 1) and the pre-split weight image kernel: instances + launchers.
#include <type_traits>
#include "conv_common.h"
#include "sp_patch_lds.h"

// --------------------------------------------------------------------------- halo patch, wave-specialised (8 waves)
// In igemm_patch_sp_body (sp_patch.h) every wave does everything: its MFMA burst is followed by the split + store of the next
// weight slab, the fragment reads and the barrier, and two waves per SIMD from two blocks do not hide that (MFMA-busy
// 0.30-0.34).  Here a 512-thread block splits the roles.  Waves 0-3 (one per SIMD) are CONSUMERS: per slab they issue
// the MFMAs of the current slab in an order that never puts two dependent products back to back, with the LDS reads
// of the NEXT slab's fragments pinned between them (sched_barrier keeps the compiler from sinking the reads to their
// uses), and nothing else.  Waves 4-7 are PRODUCERS.  The roles share their SIMD's vector issue: an MFMA leaves 8 of its 16
// cycles free, and every vector / LDS / memory instruction of EITHER wave beyond that is paid in matrix-pipe time (measured,
// DESIGN.md section 3) -- the split of roles moves the staging instructions, it does not make them free, so the producer is
// written for instruction count: the weights come PRE-SPLIT from a global image laid out slab by slab exactly like the LDS
// buffer (splitting a weight slab on the fly is ~30 instructions per thread and slab; the image is persistent, rebuilt once
// per model call) and the producers only copy them -- global -> registers two slabs ahead -> ds_write_b128 two slabs ahead of
// their first read -- and stage the next K stage's patch into the second patch buffer from per-block granule tables.  One
// barrier per slab orders both roles.  One block per CU, persistent over a range of tiles.
template <int NS, int TH, int WTN, int CS>
struct SpPatchWsLds {
  using P = SpPatchLds<NS, TH, WTN, CS>;
  static constexpr int STAT_MAXN = 1024;                           // BatchNorm statistics in the epilogue: [2][N] fp64 sums per block
  static constexpr int STAT = 2 * STAT_MAXN * 8;
  static constexpr int BYTES = 2 * P::PATCH + 3 * P::WSTAGE + STAT;       // two patch buffers, three weight slabs, the sums
  static constexpr int NSLAB = (9 * CS + 1) / 2;
};

// weight image: for every (channel tile, K stage, slab) the WSTAGE bytes the LDS weight buffer holds for it; one
// launch writes the images of all problems of a grouped launch
template <int NS, int WTN, int CS>
__device__ __forceinline__ void sp_weight_image_body(const float* __restrict__ w, unsigned char* __restrict__ img, int K,
                                                     float wscale, int blk) {
  using L = SpPatchLds<NS, 8, WTN, CS>;
  constexpr int BN = 16 * WTN, WG = BN * 8, NU = 9 * CS, NSLAB = (NU + 1) / 2;
  const int nks = K / (16 * CS);
  const int slab = blk % NSLAB;
  const int ks = (blk / NSLAB) % nks;
  const int nt = blk / (NSLAB * nks);
  unsigned char* dst = img + (size_t)blk * L::WSTAGE;
  for (int f = threadIdx.x; f < WG; f += 256) {
    const int n = f >> 3, unit = (f >> 2) & 1, gq = f & 3;
    const int u = 2 * slab + unit;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (u < NU) {
      const int t = u / CS, c = u - t * CS;
      v = *reinterpret_cast<const f32x4*>(w + ((size_t)(nt * BN + n) * 9 + t) * K + ks * CS * 16 + c * 16 + 4 * gq);
    }
    u32x2 pc[sp_np(NS)];
    sp_split4<NS>(v, pc, wscale);
    const int o = n * 64 + lds_slot(n, gq) * 16 + unit * 8;
#pragma unroll
    for (int q = 0; q < sp_np(NS); ++q) *reinterpret_cast<u32x2*>(dst + q * L::WPIECE + o) = pc[q];
  }
}
__global__ __launch_bounds__(256) void sp_weight_image_table_kernel(const WeightImageTabEntry* __restrict__ tab, int n) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int)blockIdx.x >= tab[mid].blk_end) lo = mid + 1; else hi = mid;
  }
  const WeightImageTabEntry e = tab[lo];
  const int blk = blockIdx.x - (lo ? tab[lo - 1].blk_end : 0);
  if (e.ns == 1) {
    if (e.kind == 2) sp_weight_image_body<1, 6, 3>(e.w, e.img, e.K, e.wscale, blk);
    else if (e.kind == 3) sp_weight_image_body<1, 4, 4>(e.w, e.img, e.K, e.wscale, blk);
    else sp_weight_image_body<1, 3, 3>(e.w, e.img, e.K, e.wscale, blk);
    return;
  }
  if (e.kind == 2) sp_weight_image_body<4, 6, 3>(e.w, e.img, e.K, e.wscale, blk);
  else if (e.kind == 3) sp_weight_image_body<4, 4, 4>(e.w, e.img, e.K, e.wscale, blk);
  else sp_weight_image_body<4, 3, 3>(e.w, e.img, e.K, e.wscale, blk);
}
__global__ __launch_bounds__(256) void sp_weight_image_kernel(WeightImageGroup g) {
  int gi = 0;
  while (gi + 1 < g.n && (int)blockIdx.x >= g.blk_end[gi]) ++gi;
  const int blk = blockIdx.x - (gi ? g.blk_end[gi - 1] : 0);
  const int kind = g.kind[gi];
  if (g.ns == 1) {
    if (kind == 2) sp_weight_image_body<1, 6, 3>(g.w[gi], g.img[gi], g.K[gi], g.wscale[gi], blk);
    else if (kind == 3) sp_weight_image_body<1, 4, 4>(g.w[gi], g.img[gi], g.K[gi], g.wscale[gi], blk);
    else sp_weight_image_body<1, 3, 3>(g.w[gi], g.img[gi], g.K[gi], g.wscale[gi], blk);
    return;
  }
  if (kind == 2) sp_weight_image_body<4, 6, 3>(g.w[gi], g.img[gi], g.K[gi], g.wscale[gi], blk);
  else if (kind == 3) sp_weight_image_body<4, 4, 4>(g.w[gi], g.img[gi], g.K[gi], g.wscale[gi], blk);
  else sp_weight_image_body<4, 3, 3>(g.w[gi], g.img[gi], g.K[gi], g.wscale[gi], blk);
}

// sum over the 16 lanes of a DPP row, left in lane 15 of the row (row_shr:1,2,4,8, zero fill for lanes shifted in)
__device__ __forceinline__ float sp_row16_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xf, 0xf, true));
  return v;
}

// s_waitcnt vmcnt(n) tied to the register a load fills (n: a constant once the slab loop is unrolled)
__device__ __forceinline__ void sp_wait_vm(f32x4& r, int n) {
  switch (n) {
#define HRSEG_VM(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" : "+v"(r)); break;
    HRSEG_VM(0) HRSEG_VM(1) HRSEG_VM(2) HRSEG_VM(3) HRSEG_VM(4) HRSEG_VM(5) HRSEG_VM(6) HRSEG_VM(7) HRSEG_VM(8) HRSEG_VM(9)
    HRSEG_VM(10) HRSEG_VM(11) HRSEG_VM(12) HRSEG_VM(13) HRSEG_VM(14) HRSEG_VM(15) HRSEG_VM(16) HRSEG_VM(17) HRSEG_VM(18) HRSEG_VM(19)
    HRSEG_VM(20) HRSEG_VM(21) HRSEG_VM(22) HRSEG_VM(23) HRSEG_VM(24) HRSEG_VM(25) HRSEG_VM(26) HRSEG_VM(27) HRSEG_VM(28) HRSEG_VM(29)
    HRSEG_VM(30) HRSEG_VM(31) HRSEG_VM(32) HRSEG_VM(33) HRSEG_VM(34) HRSEG_VM(35) HRSEG_VM(36) HRSEG_VM(37) HRSEG_VM(38) HRSEG_VM(39)
    HRSEG_VM(40) HRSEG_VM(41) HRSEG_VM(42) HRSEG_VM(43) HRSEG_VM(44) HRSEG_VM(45) HRSEG_VM(46) HRSEG_VM(47) HRSEG_VM(48)
#undef HRSEG_VM
    default: asm volatile("s_waitcnt vmcnt(0)" : "+v"(r)); break;
  }
}

template <int NS, int TH, int WTN, int CS, int FLIP>
__device__ __forceinline__ void igemm_patch_ws_body(const IgemmArgs& p, unsigned char* lds, const int first, const int end,
                                                    const int block_row = 0) {
  static_assert(NS == 4 || NS == 1, "the wave-specialised body: fp16x2 (two pieces, three products) or bf16 (one piece, one product)");
  using L = SpPatchLds<NS, TH, WTN, CS>;
  constexpr int RPW = TH / 4, BN = 16 * WTN, PW = 18, PP = L::PP;
  // patch granules (16 bytes of fp32 = 4 channels): a round of the 256 producer threads covers PR whole pixels,
  // thread -> (pixel ptid / GPP within the round, granule ptid % GPP of the pixel), so that a granule's pixel is
  // pix0 + PR * i with no division in the loop (CS = 3: 252 threads work, 4 idle)
  constexpr int GPP = CS * 4, PR = 256 / GPP;
  constexpr int P_LOADS = (PP + PR - 1) / PR;              // rounds per K stage
  constexpr int W16 = L::WSTAGE / 16, W_LOADS = (W16 + 255) / 256;     // 16-byte granules of a pre-split weight slab
  constexpr int NU = 9 * CS, NSLAB = (NU + 1) / 2;
#ifndef HRSEG_WS_EXP
#define HRSEG_WS_EXP 0       // MEASUREMENT ONLY (wrong results): 1 no MFMAs, 2 no weight loads, 4 no patch loads, 8 no weight stores, 16 no epilogue, 32 epilogue stores out of range
#endif
  static_assert(NSLAB % 2 == 0, "register-set parity must restart with every K stage");
  unsigned char* lpatch = lds;                             // [2][PATCH]
  unsigned char* lw = lds + 2 * L::PATCH;                  // [3][WSTAGE]
  // BatchNorm statistics of the OUTPUT in the epilogue (p.stat_partial, training forward): the block keeps [2][N] fp64 sums
  // (sum y, sum y^2 per output channel over every pixel of its tiles) in LDS and writes them as ONE row of the partial-sum
  // buffer the BatchNorm finalize kernel reads -- the statistics kernel, its launch boundary and its pass over y (measured:
  // 2.6 ms of a 51 ms step with every statistics launch left out) disappear for the layers this kernel produces.
  double* lstat = reinterpret_cast<double*>(lds + 2 * L::PATCH + 3 * L::WSTAGE);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool consumer = __builtin_amdgcn_readfirstlane(wave) < 4;      // wave-uniform: a scalar branch
  const int ptid = tid & 255;
  const int r16 = lane & 15, g = lane >> 4;
  const int H = p.Ho, W = p.Wo;
  // CANVAS mode (p.cv_w1 > 0, chosen by the host for images whose 16-column tiles are mostly padding): the cv_nb images of
  // the batch lie side by side on one canvas, a zero column between neighbours (the 3x3 halo of one image never sees the
  // next), and the tiles cover the canvas: 39 x 39 images 1.26x -> 1.05x padded area, 20 x 20 images 1.92x -> 1.32x.  A canvas
  // column cx belongs to image cx / w1 (exact multiply-high for cx, w1 < 2^16: host-checked), column cx % w1, the gap column
  // w1 - 1 = W being invalid.  Plain mode is the same arithmetic with magic 0 (image 0 of a descriptor that starts at the
  // tile's own image): one code path, results identical pixel for pixel (same K stages, slabs and product order).
  const int cv_w1 = p.cv_w1, cv_nb = p.cv_w1 > 0 ? p.cv_nb : 1;
  const unsigned cv_magic = p.cv_w1 > 0 ? p.cv_magic : 0u;
  const int Wc = p.cv_w1 > 0 ? cv_nb * cv_w1 - 1 : W;          // canvas width in pixels
  const int tiles_x = (Wc + 15) >> 4, tiles_y = (H + TH - 1) / TH;
  const int ntn = p.N / BN;
  const int nks = p.K / (16 * CS);
  if (first >= end) return;
#ifndef HRSEG_WS_STAMP
#define HRSEG_WS_STAMP 0     // MEASUREMENT ONLY: block 0's waves 0 (consumer) and 4 (producer) write the time they ARRIVE at every slab barrier
#endif                       // and the time they LEAVE it into p.stat_partial ([role][slab][2] 64-bit counters; no statistics then)
#if HRSEG_WS_STAMP
  const bool stat = false;
  unsigned long long* const stamp_out = reinterpret_cast<unsigned long long*>(p.stat_partial);
  const bool stamping = stamp_out != nullptr && block_row == 0 && (wave == 0 || wave == 4);
  int stamp_j = 0;
  auto stamped_barrier = [&]() {
    unsigned long long t0, t1;
    asm volatile("s_memtime %0" : "=s"(t0));
    __builtin_amdgcn_s_barrier();
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1));
    if (stamping && stamp_j < 1024 && lane == 0) {
      unsigned long long* o = stamp_out + ((wave >> 2) * 1024 + stamp_j) * 2;
      o[0] = t0;
      o[1] = t1;
    }
    ++stamp_j;
  };
#else
  const bool stat = p.stat_partial != nullptr;
  auto stamped_barrier = [&]() { __builtin_amdgcn_s_barrier(); };
#endif
  if (stat)
    for (int i = tid; i < 2 * p.N; i += 512) lstat[i] = 0.0;            // (ordered before the first epilogue by the prologue barrier)

  // tile t -> (channel tile fastest, then tile column, tile row, image); walked incrementally (the divisions
  // happen once per block: a producer wave has no issue slots to spare for them)
  struct Geom { int b, y0, x0, nt; };
  auto tile_geom = [&](int t) {
    Geom q;
    q.nt = t % ntn;
    int mt = t / ntn;
    const int tx = mt % tiles_x;
    mt /= tiles_x;
    const int ty = mt % tiles_y;
    q.b = mt / tiles_y;
    q.y0 = ty * TH; q.x0 = tx * 16;
    return q;
  };
  auto tile_next = [&](Geom& q) {
    if (++q.nt < ntn) return;
    q.nt = 0;
    q.x0 += 16;
    if (q.x0 < tiles_x * 16) return;
    q.x0 = 0;
    q.y0 += TH;
    if (q.y0 < tiles_y * TH) return;
    q.y0 = 0;
    ++q.b;
  };

  if (consumer) {
    float xscale, xinv;
    sp_pow2_scale(p.xmax, xscale, xinv);
    const float oscale = xinv * p.wscale_inv;
    const int foff = r16 * 64 + lds_slot(r16, g) * 16;
    const int prow0 = (wave * RPW) * PW + r16;
    const int pbase = prow0 * 32;
    constexpr int NP = sp_np(NS);
    constexpr int UNITS = RPW * NP + WTN * NP;             // fragment registers (8 halfs each) of a slab
    constexpr int MM = WTN * RPW * sp_nprod(NS);           // MFMAs of a slab
    // fragment r of slab `slab` (compile-time) -> register set
    // A pixel fragment's LDS address is (patch pixel prow0 + c) * 32 + the 8-byte slot g, swizzled by bit 3 of the pixel index,
    // c = m * PW + tap offset a compile-time constant.  The swizzle depends on c only through c mod 16, so SIXTEEN per-lane base
    // registers (xbase[j]: the lane's pixel prow0, slot swizzled for c = j mod 16, the patch buffer the reads currently target)
    // serve every fragment read with an immediate offset -- left to itself the compiler keeps one address register per
    // (row, tap) pair, ~40-57 loop-invariant registers on the 16-row tiling, which is what made these kernels spill.
    int xbase[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) xbase[j] = pbase + ((g ^ (2 * (((prow0 + j) >> 3) & 1))) << 3);
    auto xbase_flip = [&](int to_buf) {
#pragma unroll
      for (int j = 0; j < 16; ++j) xbase[j] += to_buf ? L::PATCH : -L::PATCH;
    };
    auto read_unit = [&](int slab, int wboff, int r, bf16x8 (&xf)[RPW][NP], bf16x8 (&wf)[WTN][NP]) {
      if (r < RPW * NP) {
        const int m = r / NP, q = r % NP;
        const int uA = 2 * slab, uB = 2 * slab + 1;
        const int tA = uA / CS, cA = uA - tA * CS;
        const int tB = (uB < NU) ? uB / CS : 0, cB = (uB < NU) ? uB - tB * CS : 0;
        const int dA = (FLIP ? 2 - tA / 3 : tA / 3) * PW + (FLIP ? 2 - tA % 3 : tA % 3);
        const int dB = (FLIP ? 2 - tB / 3 : tB / 3) * PW + (FLIP ? 2 - tB % 3 : tB % 3);
        const unsigned char* pb = lpatch + q * L::PPIECE;
        const int ca = m * PW + dA, cb = m * PW + dB;
        const u32x2 lo = *reinterpret_cast<const u32x2*>(pb + xbase[ca & 15] + (cA * L::CHUNK + ca * 32));
        u32x2 hi = u32x2{0u, 0u};
        if (uB < NU) hi = *reinterpret_cast<const u32x2*>(pb + xbase[cb & 15] + (cB * L::CHUNK + cb * 32));
        xf[m][q] = __builtin_bit_cast(bf16x8, (u32x4){lo[0], lo[1], hi[0], hi[1]});
      } else {
        const int i = r - RPW * NP, n = i / NP, q = i % NP;
        wf[n][q] = *reinterpret_cast<const bf16x8*>(lw + wboff + q * L::WPIECE + n * 1024 + foff);
      }
    };
    f32x4 acc[WTN][RPW];
    auto zero_acc = [&]() {
#pragma unroll
      for (int n = 0; n < WTN; ++n)
#pragma unroll
        for (int m = 0; m < RPW; ++m) acc[n][m] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    // Epilogue in two parts.  fetch_add: everything the tile's output ADDS to its accumulators -- bias, the values an
    // accumulating launch (data gradient into an existing gradient) adds to, the fused residual -- read into registers;
    // store_acc: scale, add, ReLU, store.  Every read is issued before the first store (for all the compiler knows a store
    // may alias the next read, and a read behind every store is a memory round trip each: 156 -> 140 us on the accumulating
    // data-gradient launches).  Tilings with registers to spare inside the grouped kernel's allocation (PF: 48- and 64-channel
    // tiles on 8 rows, 158 / 178 of the 246 registers the 96-channel tiling makes the kernel allocate anyway) issue fetch_add
    // S_PF slabs BEFORE the tile's last slab: a 48-channel layer has ONE K stage of 14 slabs (3.5 us) per tile, and reading
    // the accumulate values at the very end exposed a memory round trip per tile (+23 us per accumulating launch).  Same
    // arithmetic, same order: bit-identical results.
    constexpr bool PF = WTN * RPW <= 8;
    constexpr int S_PF = NSLAB > 10 ? NSLAB - 10 : 0;
    f32x4 add[RPW][WTN];
    // The epilogue's launch parameters, pinned in scalar registers: `p` lives in the kernel-argument segment, and left alone
    // the compiler re-loads its fields where they are used -- one s_load + s_waitcnt lgkmcnt(0) round trip per output row of
    // EVERY tile's epilogue, with the matrix pipe idle (a tile cost ~2 us beyond its slabs; a 48-channel layer's tile is 4.6 us
    // of slabs).  A value that went through v_readfirstlane cannot be rematerialised from memory.
    auto pin_i = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
    auto pin_p = [](const void* ptr) {
      const unsigned long long a = (unsigned long long)ptr;
      const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(a & 0xffffffffull));
      const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32));
      return (unsigned long long)lo | ((unsigned long long)hi << 32);
    };
    float* const e_y = reinterpret_cast<float*>(pin_p(p.y));
    const float* const e_bias = reinterpret_cast<const float*>(pin_p(p.bias));
    const float* const e_res = reinterpret_cast<const float*>(pin_p(p.res));
    const int e_ldy = pin_i(p.ldy), e_ldr = pin_i(p.ldr), e_acc = pin_i(p.accumulate), e_relu = pin_i(p.relu);
    const int e_early = pin_i(p.epi_early), e_stat = pin_i(stat ? 1 : 0), e_N = pin_i(p.N);
    constexpr bool SREG = PF;                                  // per-lane statistics sums kept in registers over the block's tiles
    const int e_sreg = pin_i((stat && ntn == 1) ? 1 : 0);
    f32x4 rs1[SREG ? WTN : 1], rs2[SREG ? WTN : 1];
#pragma unroll
    for (int n = 0; n < (SREG ? WTN : 1); ++n) rs1[n] = rs2[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    // Output addressing: buffer descriptors based at the tile's first image (canvas mode: the cv_nb images of the canvas), 32-bit
    // byte offsets per lane, HRSEG_BUF_OOB for a pixel outside the image -- its load returns zeros, its store writes nothing: no
    // exec-mask branch per output row and no 64-bit address arithmetic in an epilogue that runs with the matrix pipe idle.
    // (Host-checked: cv_nb * H * W * ld * 4 bytes < 2^31 for y and the residual, conv.hip ws_kind / ws_canvas.)
    const unsigned ldy4 = (unsigned)e_ldy * 4u, ldr4 = (unsigned)e_ldr * 4u;
    const int wave_rows = pin_i(wave * RPW);               // first tile row of this wave
    const unsigned g16 = (unsigned)g * 16u;                // this lane's four channels inside a 16-channel tile, bytes
    auto tile_offsets = [&](const Geom& q, unsigned ld4, unsigned (&off)[RPW]) {
      // this lane's output column: canvas column -> (image, column); invalid on the gap column and past the last image.
      // One offset per tile (two 32-bit multiplies, quarter rate), the rows of the tile a scalar stride apart.
      const int cxo = q.x0 + r16;
      const int obc = (int)__umulhi((unsigned)cxo, cv_magic);
      const int ox = cxo - obc * cv_w1;
      const bool ook = !(HRSEG_WS_EXP & 32) & (ox < W) & (obc < cv_nb);
      const int oy0 = q.y0 + wave_rows;
      const unsigned base = (unsigned)((obc * H + oy0) * W + ox) * ld4 + (unsigned)(q.nt * BN) * 4u + g16;
      const unsigned rowstep = (unsigned)W * ld4;
#pragma unroll
      for (int m = 0; m < RPW; ++m) off[m] = (ook & (oy0 + m < H)) ? base + (unsigned)m * rowstep : HRSEG_BUF_OOB;
    };
    const int e_nothing = pin_i((!p.bias && !p.accumulate && !p.res) ? 1 : 0);
    auto fetch_add = [&](const Geom& q) {
      if (e_nothing) {             // the training forward and the plain data gradient: zeros, behind ONE scalar branch (the general
#pragma unroll                    // path below spent ~700 cycles per tile on its three not-taken cases: tools/ws_stamps.py)
        for (int m = 0; m < RPW; ++m)
#pragma unroll
          for (int n = 0; n < WTN; ++n) add[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
      }
#pragma unroll
      for (int n = 0; n < WTN; ++n) {
        f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
        if (e_bias) bv = *reinterpret_cast<const f32x4*>(e_bias + q.nt * BN + 16 * n + 4 * g);
#pragma unroll
        for (int m = 0; m < RPW; ++m) add[m][n] = bv;
      }
      if (e_acc) {
        const __amdgpu_buffer_rsrc_t ry = make_rsrc(e_y + (size_t)q.b * H * W * e_ldy, (size_t)cv_nb * H * W * ldy4);
        unsigned off[RPW];
        tile_offsets(q, ldy4, off);
#pragma unroll
        for (int m = 0; m < RPW; ++m)
#pragma unroll
          for (int n = 0; n < WTN; ++n) add[m][n] += buf_load4(ry, off[m], 64 * n);
      }
      if (e_res) {
        const __amdgpu_buffer_rsrc_t rr = make_rsrc(e_res + (size_t)q.b * H * W * e_ldr, (size_t)cv_nb * H * W * ldr4);
        unsigned off[RPW];
        tile_offsets(q, ldr4, off);
#pragma unroll
        for (int m = 0; m < RPW; ++m)
#pragma unroll
          for (int n = 0; n < WTN; ++n) add[m][n] += buf_load4(rr, off[m], 64 * n);
      }
    };
    auto store_acc_as = [&](const Geom& q, auto plain_tag) {
      constexpr bool PLAIN = decltype(plain_tag)::value;
      const __amdgpu_buffer_rsrc_t ry = make_rsrc(e_y + (size_t)q.b * H * W * e_ldy, (size_t)cv_nb * H * W * ldy4);
      unsigned off[RPW];
      tile_offsets(q, ldy4, off);
      if (e_stat) {
        // per channel tile: this lane's sums over its RPW rows (fp32, RPW terms).  Pixels outside the image contribute nothing.
        // SREG (one channel tile per pixel tile and registers to spare: the 48- and 64-channel layers, whose tiles are the
        // shortest): the lane keeps adding into its own fp32 sums over ALL tiles of the block (a block walks a few dozen tiles)
        // and the cross-lane reduction happens once, at the end of the block (flush_stats).  Otherwise per tile: a 16-lane
        // row reduction over the tile's 16 columns (row_shr 1, 2, 4, 8 with zero fill: lane 15 of the row ends with the
        // total, 32 fp32 terms), then ONE fp64 LDS atomic per channel and sum from that lane.
#pragma unroll
        for (int n = 0; n < WTN; ++n) {
          f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int m = 0; m < RPW; ++m) {
            const bool ok = off[m] != HRSEG_BUF_OOB;
            const f32x4 v = PLAIN ? acc[n][m] * oscale : acc[n][m] * oscale + add[m][n];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float ve = ok ? v[e] : 0.f;
              s1[e] += ve;
              s2[e] += ve * ve;
            }
          }
          if (SREG && e_sreg) {
            rs1[n] += s1;
            rs2[n] += s2;
            continue;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            s1[e] = sp_row16_sum(s1[e]);
            s2[e] = sp_row16_sum(s2[e]);
          }
          if (r16 == 15) {
            const int c0 = q.nt * BN + 16 * n + 4 * g;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              __hip_atomic_fetch_add(lstat + c0 + e, (double)s1[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              __hip_atomic_fetch_add(lstat + e_N + c0 + e, (double)s2[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
          }
        }
      }
#pragma unroll
      for (int m = 0; m < RPW; ++m) {
#pragma unroll
        for (int n = 0; n < WTN; ++n) {
          f32x4 v = PLAIN ? acc[n][m] * oscale : acc[n][m] * oscale + add[m][n];
          if (!PLAIN && e_relu) v = relu_nan(v);
          buf_store4(ry, off[m], 64 * n, v);
        }
        // A 16-byte store reads its data registers over several cycles after it issues, and the compiler lets a packed
        // multiply of the NEXT row write them in the very next slot (measured on the plain path: the last dword of a row's
        // last store came out overwritten in the last four lanes of each row of 16, in 0.5 % of the tiles, run to run different).
        // Nothing crosses this point, and the next vector write is eight wait states away.
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 7" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    // (A specialisation for the training forward -- nothing to add, no ReLU: multiply in place and store -- measured no faster,
    // and its in-place multiplies are what exposed the store-data hazard above: one code path.)
    auto store_acc = [&](const Geom& q) { store_acc_as(q, std::false_type{}); };
    bf16x8 xfr[2][RPW][NP], wfr[2][WTN][NP];
    Geom cur = tile_geom(first);
    __syncthreads();                       // the producers' prologue: first patch, weight slabs 0 and 1
#pragma unroll
    for (int r = 0; r < UNITS; ++r) read_unit(0, 0, r, xfr[0], wfr[0]);
    zero_acc();
    int wb = 0, pb = 0;                    // weight buffer offset of the CURRENT slab, patch buffer of the CURRENT stage
    for (int t = first;; ++t) {
      bool have_next = false;
      for (int ks = 0; ks < nks; ++ks) {
        const bool last_ks = ks + 1 == nks;
        have_next = (last_ks ? t + 1 : t) < end;
#pragma unroll
        for (int s = 0; s < NSLAB; ++s) {
          const int wb1 = (wb == 2 * L::WSTAGE) ? 0 : wb + L::WSTAGE;
          // the next slab's fragments: slab s+1 of this patch, or slab 0 of the next stage's patch (complete since
          // the barrier before this slab; past the block's last stage the reads fetch stale data nobody uses)
          const int nslab = (s + 1 < NSLAB) ? s + 1 : 0;
          if (s + 1 == NSLAB) xbase_flip(pb ^ 1);          // (every read of a stage's last slab targets the next stage's patch)
          int k = 0;
#pragma unroll
          for (int pr = 0; pr < sp_nprod(NS); ++pr) {
#pragma unroll
            for (int n = 0; n < WTN; ++n) {
#pragma unroll
              for (int m = 0; m < RPW; ++m) {
                // products in the order of sp_mma (w1 x0, w0 x1, w0 x0) per accumulator, WTN*RPW MFMAs apart
                if (NS == 4) {
                  const f16x8 wv = __builtin_bit_cast(f16x8, wfr[s & 1][n][pr == 0 ? NP - 1 : 0]);
                  const f16x8 xv = __builtin_bit_cast(f16x8, xfr[s & 1][m][pr == 1 ? NP - 1 : 0]);
#if HRSEG_WS_EXP & 1
                  asm volatile("" :: "v"(wv), "v"(xv));
#else
                  acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wv, xv, acc[n][m], 0, 0, 0);
#endif
                } else {
                  acc[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr[s & 1][n][0], xfr[s & 1][m][0], acc[n][m], 0, 0, 0);
                }
                // the next slab's fragment reads, spread over this slab's MFMAs (front-loading them so that the last MFMAs cover
                // their latency measured no different: the wait before the slab barrier is not where the slab's time goes)
#pragma unroll
                for (int r = k * UNITS / MM; r < (k + 1) * UNITS / MM; ++r)
                  read_unit(nslab, wb1, r, xfr[(s + 1) & 1], wfr[(s + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
                ++k;
              }
            }
          }
#if HRSEG_WS_EXP & 16
          if (s == NSLAB - 1 && last_ks) {
            if (acc[0][0][0] == 1.2345f) store_acc(cur);
            zero_acc();
          }
#else
          if (PF && s == S_PF && last_ks && e_early) fetch_add(cur);
          if (s == NSLAB - 1 && last_ks) {
#if HRSEG_WS_STAMP
            unsigned long long e0, e1, e2, e3;                // (measurement build: the epilogue's phases of wave 0, block 0)
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(e0) :: "memory");
            if (!(PF && e_early)) fetch_add(cur);
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(e1) :: "memory");
            store_acc(cur);
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(e2) :: "memory");
            zero_acc();
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(e3) :: "memory");
            if (stamping && wave == 0 && lane == 0 && stamp_j < 1024) {
              unsigned long long* o = stamp_out + 4096 + stamp_j * 4;
              o[0] = e0; o[1] = e1; o[2] = e2; o[3] = e3;
            }
#else
            if (!(PF && e_early)) fetch_add(cur);
            store_acc(cur);
            zero_acc();
#endif
          }
#endif
          // The slab barrier orders LDS traffic only (the producers' ds_writes against these reads).  __syncthreads() would
          // also wait for every outstanding vector-memory operation of this wave (its workgroup-scope fence emits vmcnt(0)):
          // the tile's stores after store_acc -- a memory round trip per tile before the next tile's first slab -- and the
          // loads of fetch_add issued S_PF slabs early.  Nothing another wave of the block reads depends on them, so the
          // consumers wait for their LDS operations and meet the barrier directly.
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          stamped_barrier();
          wb = wb1;
        }
        pb ^= 1;
        if (last_ks) tile_next(cur);
      }
      if (!have_next) break;
    }
    if (SREG && e_sreg) {          // the register sums of this wave: row reduction, then one fp64 LDS atomic per channel and sum
#pragma unroll
      for (int n = 0; n < WTN; ++n) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float a = sp_row16_sum(rs1[n][e]), b = sp_row16_sum(rs2[n][e]);
          if (r16 == 15) {
            __hip_atomic_fetch_add(lstat + 16 * n + 4 * g + e, (double)a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(lstat + e_N + 16 * n + 4 * g + e, (double)b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          }
        }
      }
    }
  } else {
    // PRODUCERS.  A wave issues an instruction every four or five cycles at best and the block meets at ONE barrier per slab, so a
    // slab lasts as long as its slowest wave's instruction stream: a 36-MFMA slab is 576 cycles of the matrix pipe, i.e. ~120
    // producer instructions.  (Round 4 measured the previous flat-loop producer -- ~230 instructions per slab on the 16-row
    // tiling, a third of them per-granule address arithmetic with quarter-rate 32-bit multiplies -- as what set the slab time:
    // 2,240 / 1,340-1,710 cycles per slab on 16-row / 96-channel tiles, 1,450 / 990-1,140 with the loads and their address
    // arithmetic compiled out, tools/ws_bound.py.)  This producer runs K stage by K stage with the slab loop of a stage unrolled
    // (every condition on the slab index folds away), and everything about a patch granule that does not depend on the tile --
    // its pixel of the patch, its offset from the patch origin, its LDS address -- is computed ONCE per block:
    //   * weights: slab j+2 goes from the register ring (loaded D slabs earlier) to LDS, slab j+2+D is loaded into the same
    //     registers: one address add per load / store group, the image offset of the stage is a scalar;
    //   * patch of the NEXT stage, granule by granule (loaded at slab s, split and stored at slab s+D): an interior tile's
    //     granule loads with its precomputed offset as the vector offset and the tile origin as the scalar offset -- no
    //     vector instruction at all; a border or canvas tile pays eight (row / column range tests against per-stage scalars);
    //   * waits are counted: the number of loads younger than the one a store needs is a compile-time function of the slab.
    float xscale, xinv;
    sp_pow2_scale(p.xmax, xscale, xinv);
    const int per_tile = nks * NSLAB;                      // slabs (= weight image entries) per tile
    auto rsrc_words = [](const void* base, size_t bytes) {
      const unsigned long long a = (unsigned long long)base;
      i32x4_t r;
      r[0] = (int)(unsigned)(a & 0xffffffffull);
      r[1] = (int)(unsigned)((a >> 32) & 0xffffull);
      r[2] = (int)(unsigned)(bytes > 0xFFFFFFFFull ? 0xFFFFFFFFull : bytes);
      r[3] = HRSEG_BUF_FLAGS;
      return r;
    };
    auto ld16 = [](f32x4& dst, const i32x4_t& rs, unsigned voff, unsigned soff) {
      asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=&v"(dst) : "v"(voff), "s"(rs), "s"(soff) : "memory");
    };
    const i32x4_t rw = rsrc_words(p.wimg, (size_t)ntn * per_tile * L::WSTAGE);
    // ---- what a thread's patch granules are, once per block
    const int pix0 = ptid / GPP, prem = ptid - pix0 * GPP;
    const bool pwork = pix0 < PR;                          // (CS = 3: the last four threads stage no patch granule)
    const int pst0 = (prem >> 2) * L::CHUNK, pq = prem & 3;
    const unsigned ldx4 = (unsigned)p.ldx * 4u;
    unsigned rel[P_LOADS];          // byte offset of the granule from the patch origin (row y0-1, column x0-1) of a plain image
    int lst[P_LOADS];               // its LDS byte offset inside a patch buffer (piece 0)
    int gpy[P_LOADS], gpx[P_LOADS]; // its patch row and column (row: a value no image reaches for a granule that does not exist)
#pragma unroll
    for (int i = 0; i < P_LOADS; ++i) {
      const int pix = pix0 + PR * i;
      const int py = (pix * 3641) >> 16, px = pix - py * PW;           // pix / 18 for pix < 2^12
      const bool ex = pwork & (pix < PP);
      rel[i] = ex ? (unsigned)(py * W + px) * ldx4 + (unsigned)prem * 16u : HRSEG_BUF_OOB;
      // a granule that does not exist stores zeros into the padding behind chunk 0's pixels (CHUNK is PP * 32 + 192 bytes)
      lst[i] = ex ? pst0 + pix * 32 + ((pq ^ (2 * ((pix >> 3) & 1))) << 3) : PP * 32 + (lane & 15) * 8;
      gpy[i] = ex ? py : 0x40000000;
      gpx[i] = px;
    }
    static_assert(L::CHUNK - PP * 32 >= 128 + 8, "the padding of a chunk image takes the stores of granules that do not exist");
    // weights: 16-byte granule f = ptid + 256 i of a slab
    unsigned wv[W_LOADS];
#pragma unroll
    for (int i = 0; i < W_LOADS; ++i) wv[i] = (ptid + 256 * i < W16) ? (unsigned)(ptid + 256 * i) * 16u : 0x80000000u;
    const bool wlast = __builtin_amdgcn_readfirstlane((int)((wave - 4) * 64 + 256 * (W_LOADS - 1) < W16)) != 0;   // wave-uniform
    const int wl0 = (int)(lw - lds) + ptid * 16;
    const int exp_nosplit = p.exp_nosplit | p.x_presplit;        // x stored pre-split: copy, do not split (see hrseg.h x_split)
    // ---- per-stage scalars of the stage whose patch is being staged
    struct Stage { unsigned tb, tb0, delta; int y0m1, x0m1, xlo, xspan, xb; bool fast, second; };
    const unsigned hw = (unsigned)(H * W);
    auto stage_scalars = [&](const Geom& q) {
      Stage z;
      const int x0m1 = q.x0 - 1;
      z.y0m1 = q.y0 - 1;
      z.x0m1 = x0m1;
      z.xlo = x0m1 < 0 ? 1 : 0;
      if (cv_w1 > 0) {
        const int bc0 = x0m1 < 0 ? 0 : (int)__umulhi((unsigned)x0m1, cv_magic);
        z.xb = (bc0 + 1) * cv_w1 - x0m1;
        z.second = bc0 + 1 < cv_nb;
        z.tb0 = ((unsigned)((bc0 * H + z.y0m1) * W + x0m1 - bc0 * cv_w1)) * ldx4;
        z.delta = (hw - (unsigned)cv_w1) * ldx4;
        z.fast = false;
        if (bc0 >= cv_nb) z.xb = z.xlo + 1;               // (a tile column past the last image: nothing valid)
      } else {
        z.xb = W - x0m1 + 1;
        z.second = false;
        z.tb0 = (unsigned)(z.y0m1 * W + x0m1) * ldx4;
        z.delta = 0u;
        z.fast = (q.y0 >= 1) & (q.y0 + TH + 1 <= H) & (q.x0 >= 1) & (q.x0 + 17 <= W);
      }
      z.xspan = z.xb - 1 - z.xlo;
      z.tb = z.tb0;
      return z;
    };
    const bool cv_narrow = cv_w1 > 0 && cv_w1 < 18;       // an 18-column patch may span three images: exact per-granule arithmetic
    auto patch_voff = [&](const Stage& z, int i) -> unsigned {          // border / canvas tile: the granule's offset or OOB
      if (cv_narrow) {
        const int iy = gpy[i] + z.y0m1, cx = gpx[i] + z.x0m1;
        const int bc = (int)__umulhi((unsigned)cx, cv_magic);
        const int ix = cx - bc * cv_w1;
        const bool ok = ((unsigned)iy < (unsigned)H) & (cx >= 0) & (ix < W) & (bc < cv_nb);
        return ok ? (unsigned)((bc * H + iy) * W + ix) * ldx4 + (unsigned)prem * 16u : HRSEG_BUF_OOB;
      }
      const bool oky = (unsigned)(gpy[i] + z.y0m1) < (unsigned)H;
      const bool ok1 = (unsigned)(gpx[i] - z.xlo) < (unsigned)z.xspan;
      const bool ok2 = z.second & (gpx[i] >= z.xb);
      const unsigned off = rel[i] + z.tb0 + (ok2 ? z.delta : 0u);
      return (oky & (ok1 | ok2)) ? off : HRSEG_BUF_OOB;
    };
    auto patch_store1 = [&](const f32x4& v, int i, int pboff) {
      u32x2 pc[sp_np(NS)];
      if (exp_nosplit) {
        const u32x4 raw = __builtin_bit_cast(u32x4, v);
#pragma unroll
        for (int s = 0; s < sp_np(NS); ++s) pc[s] = u32x2{raw[(2 * s) & 3], raw[(2 * s + 1) & 3]};
      } else {
        sp_split4<NS>(v, pc, xscale);
      }
      const int o = pboff + lst[i];
#pragma unroll
      for (int s = 0; s < sp_np(NS); ++s) *reinterpret_cast<u32x2*>(lpatch + s * L::PPIECE + o) = pc[s];
    };
    auto image_rsrc = [&](int b) { return rsrc_words(p.x + (size_t)b * H * W * p.ldx, (size_t)cv_nb * H * W * p.ldx * 4); };
    // image offset of the weight slabs of stage (channel tile nt, K stage ks)
    auto stage_woff = [&](int nt, int ks) { return (unsigned)((nt * nks + ks) * NSLAB) * (unsigned)L::WSTAGE; };
    // Registers in flight.  Weights: a ring of DW = 2 slab sets -- a stage has an even number of slabs, so every stage starts at
    // ring position 0 and the loop's back edge maps each register to itself.  (The loads are inline assembly the compiler knows
    // nothing about: a ring whose phase alternates between stages needs two code instances and a join between them, and at
    // that join the compiler MOVED ring registers whose loads were still in flight -- measured, wrong results.)  Patch: one
    // register set per granule of the stage, loaded GPL per slab from slab 0 and stored DP slabs later -- nothing of it is in
    // flight across a stage boundary.
    constexpr int DW = 2;
    constexpr int GPL = (P_LOADS + NSLAB - 6) / (NSLAB - 5);           // granules loaded per slab so that DP >= 4
    constexpr int DP = NSLAB - 1 - (P_LOADS + GPL - 1) / GPL;          // the last granule is stored at slab NSLAB - 2
    static_assert(DP >= 4 && (P_LOADS + GPL - 1) / GPL <= NSLAB - DW, "patch schedule");
    f32x4 rw4[DW][W_LOADS], pg[P_LOADS];
    Geom cur = tile_geom(first);
    // ---- prologue: the first patch and weight slabs 0, 1 into LDS, slabs 2 .. D+1 in flight
    unsigned woff_cur = stage_woff(cur.nt, 0);             // weight image offset of the CURRENT stage's slab 0
    {
      f32x4 v[P_LOADS];
      const i32x4_t rx0 = image_rsrc(cur.b);
      const Stage z0 = stage_scalars(cur);
#pragma unroll
      for (int i = 0; i < P_LOADS; ++i) ld16(v[i], rx0, patch_voff(z0, i), 0u);
      f32x4 w01[2][W_LOADS];
#pragma unroll
      for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int i = 0; i < W_LOADS; ++i) ld16(w01[d][i], rw, wv[i] + woff_cur + (unsigned)(d * L::WSTAGE), 0u);
#pragma unroll
      for (int i = 0; i < P_LOADS; ++i) asm volatile("s_waitcnt vmcnt(0)" : "+v"(v[i]));
#pragma unroll
      for (int i = 0; i < P_LOADS; ++i) patch_store1(v[i], i, 0);
#pragma unroll
      for (int i = 0; i < W_LOADS; ++i) asm volatile("s_waitcnt vmcnt(0)" : "+v"(w01[0][i]), "+v"(w01[1][i]));
#pragma unroll
      for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int i = 0; i < W_LOADS; ++i)
          if (i + 1 < W_LOADS || wlast) *reinterpret_cast<f32x4*>(lds + wl0 + d * L::WSTAGE + i * 4096) = w01[d][i];
    }
    // the stage after the current one (its patch is staged during the current stage; its weights follow the current stage's)
    int n_t = first, n_ks = 0;
    Geom nxt = cur;
    i32x4_t rxn = image_rsrc(cur.b);
    bool have_next = false;
    unsigned woff_nxt = 0u;
    auto advance = [&]() {                  // nxt := the stage after nxt
      if (++n_ks == nks) {
        n_ks = 0;
        ++n_t;
        const int b = nxt.b;
        tile_next(nxt);
        if (nxt.b != b) rxn = image_rsrc(nxt.b);
      }
      have_next = n_t < end;
      woff_nxt = stage_woff(nxt.nt, n_ks);
    };
    advance();
    // slab k (0 <= k < 2 NSLAB, counted from the current stage's slab 0) -> its byte offset in the weight image
    auto slab_woff = [&](int k) { return k < NSLAB ? woff_cur + (unsigned)(k * L::WSTAGE) : woff_nxt + (unsigned)((k - NSLAB) * L::WSTAGE); };
    static_assert(2 + 2 * DW <= NSLAB, "weight look-ahead stays within the next stage");
#pragma unroll
    for (int d = 0; d < DW; ++d)
#pragma unroll
      for (int i = 0; i < W_LOADS; ++i) ld16(rw4[(d + 2) % DW][i], rw, wv[i] + slab_woff(d + 2), 0u);
    __syncthreads();
    int wb2 = 2 * L::WSTAGE;               // LDS weight buffer of slab j+2
    int pboff = 0;                         // patch buffer of the current stage (byte offset)
    // loads of slab s, in issue order: W_LOADS weight loads, then nl(s) patch loads (granules s GPL .. of the next stage's patch)
    auto nl = [](int s) { s = ((s % NSLAB) + NSLAB) % NSLAB; const int r = P_LOADS - s * GPL; return r < 0 ? 0 : (r > GPL ? GPL : r); };
    const int nstages = (end - first) * nks;
    int q = 0;
    do {                                    // one K stage per iteration (at least one: first < end)
      const Stage z = stage_scalars(nxt);
      const i32x4_t rx = have_next ? rxn : rsrc_words(p.x, 0);       // (no next stage: a descriptor of size 0, every load out of range)
      const unsigned soff = z.tb + (unsigned)(n_ks * CS * 64);
      const unsigned ksoff = (unsigned)(n_ks * CS * 64);
#pragma unroll
      for (int s = 0; s < NSLAB; ++s) {
        // ---- weights: slab s+2 -> LDS, slab s+2+DW -> registers
        {
          int yw = nl(s - DW);
#pragma unroll
          for (int k = s - DW + 1; k < s; ++k) yw += W_LOADS + nl(k);
          f32x4 (&wset)[W_LOADS] = rw4[s % DW];
#pragma unroll
          for (int i = 0; i < W_LOADS; ++i) sp_wait_vm(wset[i], yw);
          const int a = wl0 + wb2;
#pragma unroll
          for (int i = 0; i < W_LOADS; ++i)
            if (!(HRSEG_WS_EXP & 8) && (i + 1 < W_LOADS || wlast)) *reinterpret_cast<f32x4*>(lds + a + i * 4096) = wset[i];
          const unsigned wo = slab_woff(s + 2 + DW);
#pragma unroll
          for (int i = 0; i < W_LOADS; ++i) ld16(wset[i], rw, (HRSEG_WS_EXP & 2) ? HRSEG_BUF_OOB : wv[i], wo);     // (slab offset: scalar)
        }
        // ---- patch of the next stage: the granules loaded at slab s-DP are stored, nl(s) granules are loaded
        if (s >= DP && nl(s - DP) > 0) {
          int yp = W_LOADS;
#pragma unroll
          for (int k = s - DP + 1; k < s; ++k) yp += W_LOADS + nl(k);
#pragma unroll
          for (int e = 0; e < GPL; ++e)
            if (e < nl(s - DP)) sp_wait_vm(pg[(s - DP) * GPL + e], yp + nl(s - DP) - 1 - e);
          if (have_next) {
#pragma unroll
            for (int e = 0; e < GPL; ++e)
              if (e < nl(s - DP)) patch_store1(pg[(s - DP) * GPL + e], (s - DP) * GPL + e, L::PATCH - pboff);
          }
        }
#pragma unroll
        for (int e = 0; e < GPL; ++e) {
          if (e < nl(s)) {
            const int i = s * GPL + e;
            if (HRSEG_WS_EXP & 4) ld16(pg[i], rx, HRSEG_BUF_OOB, 0u);
            else if (z.fast) ld16(pg[i], rx, rel[i], soff);
            else ld16(pg[i], rx, patch_voff(z, i), ksoff);
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (the LDS stores; the loads in flight stay in flight)
        stamped_barrier();
        wb2 = (wb2 == 2 * L::WSTAGE) ? 0 : wb2 + L::WSTAGE;
      }
      pboff = L::PATCH - pboff;
      woff_cur = woff_nxt;
      advance();
    } while (++q < nstages);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the look-ahead loads of slabs past the block's last
  }
  if (stat) {
    // every consumer has added its last tile (LDS atomics complete before the barrier); the block's sums go out as row
    // `block_row` of the partial buffer [rows][2][N], which the BatchNorm finalize phase (hrseg_bn_fwd_group_phases) adds up in row order
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    double* row = p.stat_partial + (size_t)block_row * 2 * p.N;
    for (int i = tid; i < 2 * p.N; i += 512) row[i] = lstat[i];
  }
}

template <int NS, int TH, int WTN, int CS, int FLIP>
__global__ __launch_bounds__(512) void igemm_patch_ws_kernel(IgemmArgs p, int ntotal) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[SpPatchWsLds<NS, TH, WTN, CS>::BYTES];
  const int chunk = (ntotal + gridDim.x - 1) / gridDim.x;
  const int first = blockIdx.x * chunk;
  igemm_patch_ws_body<NS, TH, WTN, CS, FLIP>(p, lds, first, min(first + chunk, ntotal), blockIdx.x);
}

// grouped form: every problem runs the wave-specialised body on its own range of persistent blocks (grp.tiles[g]
// blocks for problem g, grp.ksplit[g] = its tile count), with its own channel tiling: kind 1 = 48 channels x 48-channel
// K stages, 2 = 96 x 48, 3 = 64 x 64, 4 = 48 x 48 on 16-row tiles
template <int NS, int FLIP>
__global__ __launch_bounds__(512) void igemm_patch_ws_group_kernel(IgemmGroup grp) {
  static_assert(SpPatchWsLds<NS, 16, 3, 3>::BYTES >= SpPatchWsLds<NS, 8, 4, 4>::BYTES &&
                SpPatchWsLds<NS, 16, 3, 3>::BYTES >= SpPatchWsLds<NS, 8, 6, 3>::BYTES, "LDS of the largest variant");
  __shared__ __attribute__((aligned(16))) unsigned char lds[SpPatchWsLds<NS, 16, 3, 3>::BYTES];
  int gi = 0;
  while (gi + 1 < grp.n && (int)blockIdx.x >= grp.blk_end[gi]) ++gi;
  const int local = blockIdx.x - (gi ? grp.blk_end[gi - 1] : 0);
  const int nblk = grp.tiles[gi], ntotal = grp.ksplit[gi];
  const int chunk = (ntotal + nblk - 1) / nblk;
  const int first = local * chunk, end = min(first + chunk, ntotal);
  const int kind = grp.kind[gi];
  if (kind == 1) igemm_patch_ws_body<NS, 8, 3, 3, FLIP>(grp.a[gi], lds, first, end, local);
  else if (kind == 2) igemm_patch_ws_body<NS, 8, 6, 3, FLIP>(grp.a[gi], lds, first, end, local);
  else if (kind == 3) igemm_patch_ws_body<NS, 8, 4, 4, FLIP>(grp.a[gi], lds, first, end, local);
  else igemm_patch_ws_body<NS, 16, 3, 3, FLIP>(grp.a[gi], lds, first, end, local);
}

// --------------------------------------------------------------------------- launchers
int launch_weight_images(const WeightImageGroup& g, int nblocks, hipStream_t st) {
  hipLaunchKernelGGL(sp_weight_image_kernel, dim3(nblocks), dim3(256), 0, st, g);
  return 0;
}
int launch_weight_image_table(const WeightImageTabEntry* tab, int n, int nblocks, hipStream_t st) {
  hipLaunchKernelGGL(sp_weight_image_table_kernel, dim3(nblocks), dim3(256), 0, st, tab, n);
  return 0;
}
int launch_ws_kernel(const IgemmArgs& a, int kind, int flip, int blocks, int ntotal, hipStream_t st, int ns) {
  const dim3 grid((unsigned)blocks);
#define WS1(NS_, K_, H_, N_, C_) if (ns == NS_ && kind == K_) { \
    if (flip) hipLaunchKernelGGL((igemm_patch_ws_kernel<NS_, H_, N_, C_, 1>), grid, dim3(512), 0, st, a, ntotal); \
    else hipLaunchKernelGGL((igemm_patch_ws_kernel<NS_, H_, N_, C_, 0>), grid, dim3(512), 0, st, a, ntotal); \
    return 0; }
  WS1(4, 1, 8, 3, 3) WS1(4, 2, 8, 6, 3) WS1(4, 3, 8, 4, 4) WS1(4, 4, 16, 3, 3)
  WS1(1, 1, 8, 3, 3) WS1(1, 2, 8, 6, 3) WS1(1, 3, 8, 4, 4) WS1(1, 4, 16, 3, 3)      // bf16: one piece, one product
#undef WS1
  return 1;
}
int launch_ws_group_kernel(const IgemmGroup& g, int flip, hipStream_t st, int ns) {
  const int end = g.blk_end[g.n - 1];
  if (ns == 1) {
    if (flip) hipLaunchKernelGGL((igemm_patch_ws_group_kernel<1, 1>), dim3(end), dim3(512), 0, st, g);
    else hipLaunchKernelGGL((igemm_patch_ws_group_kernel<1, 0>), dim3(end), dim3(512), 0, st, g);
    return 0;
  }
  if (flip) hipLaunchKernelGGL((igemm_patch_ws_group_kernel<4, 1>), dim3(end), dim3(512), 0, st, g);
  else hipLaunchKernelGGL((igemm_patch_ws_group_kernel<4, 0>), dim3(end), dim3(512), 0, st, g);
  return 0;
}
