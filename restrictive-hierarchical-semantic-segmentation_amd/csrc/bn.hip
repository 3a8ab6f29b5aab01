// Batch-norm (training statistics, apply, backward; grouped: n problems per launch) and the level heads fused into
// its backward, on NHWC fp32 for gfx950.  All HBM-bound: one pass per tensor, 16-byte accesses, per-channel parameters
// held in registers.  Thread mapping: elem_common.h.
#include <type_traits>
#include "elem_common.h"
#include "sp_arith.h"      // the pre-split activation granule: hrseg_split_f16x2 / hrseg_join_f16x2

// Sum of partial[k][which][c] over chunks k for the block's 16 channels: 16 chunk lanes per
// channel (a serial loop over up to 1024 chunks is a chain of dependent HBM-latency loads).
// Returns the totals to the threads with lane==0 (tid < 16).
__device__ __forceinline__ void reduce_chunks16(const double* __restrict__ partial, int nchunks, int C, int c,
                                               double& s0, double& s1, double* red) {
  const int lane = threadIdx.x >> 4;  // 0..15
  double a = 0.0, b = 0.0;
  if (c < C) {
    // up to 16 chunks per lane: issue the loads in batches of 4 chunks (8 independent loads in flight)
    // instead of a load-add chain of cold-memory latencies
    int k = lane;
    for (; k + 48 < nchunks; k += 64) {
      double t0[4], t1[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        t0[u] = partial[((size_t)(k + 16 * u) * 2 + 0) * C + c];
        t1[u] = partial[((size_t)(k + 16 * u) * 2 + 1) * C + c];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a += t0[u];
        b += t1[u];
      }
    }
    for (; k < nchunks; k += 16) {
      a += partial[((size_t)k * 2 + 0) * C + c];
      b += partial[((size_t)k * 2 + 1) * C + c];
    }
  }
  red[threadIdx.x * 2] = a;
  red[threadIdx.x * 2 + 1] = b;
  __syncthreads();
  s0 = 0.0;
  s1 = 0.0;
  if (threadIdx.x < 16)
    for (int l = 0; l < 16; ++l) {
      s0 += red[(l * 16 + threadIdx.x) * 2];
      s1 += red[(l * 16 + threadIdx.x) * 2 + 1];
    }
}

// BatchNorm (running statistics) folded into the preceding convolution's weights and bias: block = one output channel
__global__ __launch_bounds__(256) void bn_fold_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ rmean, const float* __restrict__ rvar, float eps,
                                                      int row, float* __restrict__ w_out, float* __restrict__ b_out) {
  const int co = blockIdx.x;
  const float s = (gamma ? gamma[co] : 1.f) / sqrtf(rvar[co] + eps);
  for (int i = threadIdx.x; i < row; i += 256) w_out[(size_t)co * row + i] = w[(size_t)co * row + i] * s;
  if (threadIdx.x == 0) b_out[co] = ((bias ? bias[co] : 0.f) - rmean[co]) * s + (beta ? beta[co] : 0.f);
}

// =========================================================================== grouped batch norm
// n independent BatchNorm problems (the parallel HRNet branches, or just one) per launch: block
// ranges [blk_end[g-1], blk_end[g]) belong to problem g.  Three launches forward (statistics,
// finalize, apply) and three backward (reduce, finalize, apply) whatever n is.  (Folding the finalize
// into the statistics kernel was measured slower three times -- last block reducing cold partials: 2-3x; fp64
// atomics into one accumulator: blocks finishing together serialise on 2*C addresses; sixteen accumulator rows and
// a last block that only adds those up (bn_last_block below, kept as an opt-in): +0.8 ms per step -- see DESIGN.md.)
#define BN_MAXG 8
struct BnGroupHdr { int n; int blk_end[BN_MAXG]; };
__device__ __forceinline__ int bn_find(const BnGroupHdr& h, int& local, int& nblk) {
  int g = 0;
  while (g + 1 < h.n && (int)blockIdx.x >= h.blk_end[g]) ++g;
  const int lo = g ? h.blk_end[g - 1] : 0;
  local = blockIdx.x - lo;
  nblk = h.blk_end[g] - lo;
  return g;
}
struct BnFwdG { BnGroupHdr h; hrseg_bn_fwd_t p[BN_MAXG]; };
struct BnBwdG { BnGroupHdr h; hrseg_bn_bwd_t p[BN_MAXG]; };

template <bool MASK>
__device__ __forceinline__ void stats_body(const float* __restrict__ a0, int ld0, const float* __restrict__ zmask,
                                           int ldz, int relu, const float* __restrict__ yy, int ldy,
                                           const float* __restrict__ coef, long npix, int C,
                                           double* __restrict__ partial, int chunk, int nchunks, bool bwd,
                                           double* red, int nseg = 1, const unsigned char* __restrict__ bmask = nullptr) {
  // forward: sums of a0 and a0^2; backward: sums of g and g*xhat with g = a0 * (zmask > 0 if relu)
  // nseg > 1: the pixel range is nseg equal segments (the batched level passes); a chunk never
  // straddles two segments (nchunks is a multiple of nseg)
  const Lanes L = make_lanes(C);
  const int cps = nchunks / nseg, seg = chunk / cps;
  const long seg_pix = npix / nseg;
  const long per = (seg_pix + cps - 1) / cps;
  const long lo = seg * seg_pix + (long)(chunk - seg * cps) * per;
  const long seg_end = (seg + 1) * seg_pix;
  const long hi = (lo + per < seg_end) ? lo + per : seg_end;
  f32x4 s = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
  if (L.active) {
    f32x4 mean = {0.f, 0.f, 0.f, 0.f}, rstd = {1.f, 1.f, 1.f, 1.f}, sc = mean, sh = mean;
    if (bwd) {
      mean = ld4(coef + 4 * L.cq);
      rstd = ld4(coef + C + 4 * L.cq);
      sc = ld4(coef + 2 * C + 4 * L.cq);
      sh = ld4(coef + 3 * C + 4 * L.cq);
    }
    // four pixels per trip, all loads issued before the first use: a chunk is walked by few threads, so the
    // bytes in flight per CU (what HBM-bound code lives on) come from this unrolling
    constexpr int U = 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (long pix0 = lo + L.pl; pix0 < hi; pix0 += (long)U * L.P) {
      f32x4 v[U], yv[U], zz[U];      // (zz[u][0] carries the mask byte when the layer has one)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long pix = pix0 + (long)u * L.P;
        const bool ok = pix < hi;
        v[u] = ok ? ld4(a0 + pix * ld0 + 4 * L.cq) : zero;
        if (bwd) {
          yv[u] = ok ? ld4(yy + pix * ldy + 4 * L.cq) : mean;
          if (MASK && relu && bmask) zz[u][0] = __uint_as_float(ok ? (unsigned)bmask[pix * L.Q + L.cq] : 0u);
          else if (relu && zmask) zz[u] = ok ? ld4(zmask + pix * ldz + 4 * L.cq) : zero;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (!bwd) {
          s += v[u];
          s2 += v[u] * v[u];
        } else {
          f32x4 gv = v[u];
          if (MASK && relu && bmask) {
            const unsigned bm = __float_as_uint(zz[u][0]);
#pragma unroll
            for (int j = 0; j < 4; ++j) gv[j] = ((bm >> j) & 1u) ? gv[j] : 0.f;
          } else if (relu) {
            // z not given: the forward had no residual, so z > 0 <=> y*scale+shift > 0 (4 bytes less per element)
            const f32x4 zc = zmask ? zz[u] : bn_affine(yv[u], sc, sh);
#pragma unroll
            for (int j = 0; j < 4; ++j) gv[j] = zc[j] > 0.f ? gv[j] : 0.f;
          }
          const f32x4 xh = (yv[u] - mean) * rstd;
          s += gv;
          s2 += gv * xh;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    red[threadIdx.x * 8 + j] = s[j];
    red[threadIdx.x * 8 + 4 + j] = s2[j];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    double a = 0.0, b = 0.0;
    for (int pl = 0; pl < L.P; ++pl) {
      const int t = pl * L.Q + (c >> 2);
      a += red[t * 8 + (c & 3)];
      b += red[t * 8 + 4 + (c & 3)];
    }
    partial[((size_t)chunk * 2 + 0) * C + c] = a;
    partial[((size_t)chunk * 2 + 1) * C + c] = b;
  }
}

__device__ __forceinline__ void bn_finalize_channel(const hrseg_bn_fwd_t& p, int c, double s, double ss) {
  const int C = p.C;
  // stat_updates > 1: the same batch statistics enter the running averages that many times (the level
  // passes of the hierarchical models run as one) -- sequential updates, bit for bit
  const int reps = p.stat_updates > 1 ? p.stat_updates : 1;
  const long npix = p.npix * (p.stat_ranks > 1 ? p.stat_ranks : 1);      // cross-rank statistics: sums over all ranks' pixels
  const double mean = s / (double)npix;
  double var = ss / (double)npix - mean * mean;
  if (var < 0.0) var = 0.0;
  const float rstd = (float)(1.0 / sqrt(var + (double)p.eps));
  const float ga = p.gamma ? p.gamma[c] : 1.f, be = p.beta ? p.beta[c] : 0.f;
  p.coef[c] = (float)mean;
  p.coef[C + c] = rstd;
  p.coef[2 * C + c] = ga * rstd;
  p.coef[3 * C + c] = be - (float)mean * ga * rstd;
  if (p.running_mean) {
    float rm = p.running_mean[c];
    for (int r = 0; r < reps; ++r) rm = (1.f - p.momentum) * rm + p.momentum * (float)mean;
    p.running_mean[c] = rm;
  }
  if (p.running_var) {
    // stat_div > 1: the tensor holds stat_div identical copies of the pass's images (batched level
    // passes); mean and biased variance of the copies are those of one pass, the unbiased factor uses
    // one pass's pixel count
    const long n1 = npix / (p.stat_div > 1 ? p.stat_div : 1);
    const double unb = (n1 > 1) ? var * (double)n1 / (double)(n1 - 1) : var;
    float rv = p.running_var[c];
    for (int r = 0; r < reps; ++r) rv = (1.f - p.momentum) * rv + p.momentum * (float)unb;
    p.running_var[c] = rv;
  }
}

__global__ __launch_bounds__(256) void bn_stats_group_kernel(BnFwdG g) {
  __shared__ double red[256 * 8];
  int local, nblk;
  const hrseg_bn_fwd_t& p = g.p[bn_find(g.h, local, nblk)];
  stats_body<false>(p.y, p.ldy, nullptr, 0, 0, nullptr, 0, nullptr, p.npix, p.C, p.partial, local, p.nchunks, false, red, 1);
}

__global__ __launch_bounds__(256) void bn_finalize_group_kernel(BnFwdG g) {
  __shared__ double red[512];
  int local, nblk;
  const hrseg_bn_fwd_t& p = g.p[bn_find(g.h, local, nblk)];
  const int C = p.C, c = local * 16 + (threadIdx.x & 15);
  double s, ss;
  reduce_chunks16(p.partial, p.nchunks, C, c, s, ss, red);
  if (local == 0 && threadIdx.x == 0 && p.num_batches_tracked)
    *(long long*)p.num_batches_tracked += (p.stat_updates > 1 ? p.stat_updates : 1);
  if (threadIdx.x >= 16 || c >= C) return;
  bn_finalize_channel(p, c, s, ss);
}

__global__ void bn_eval_coef_group_kernel(BnFwdG g) {
  int local, nblk;
  const hrseg_bn_fwd_t& p = g.p[bn_find(g.h, local, nblk)];
  const int c = local * 64 + threadIdx.x, C = p.C;
  if (c >= C) return;
  const float rstd = 1.f / sqrtf(p.running_var[c] + p.eps);
  const float ga = p.gamma ? p.gamma[c] : 1.f, be = p.beta ? p.beta[c] : 0.f;
  p.coef[c] = p.running_mean[c];
  p.coef[C + c] = rstd;
  p.coef[2 * C + c] = ga * rstd;
  p.coef[3 * C + c] = be - p.running_mean[c] * ga * rstd;
}

__global__ __launch_bounds__(256) void bn_apply_group_kernel(BnFwdG g) {
  int local, nblk;
  const hrseg_bn_fwd_t& p = g.p[bn_find(g.h, local, nblk)];
  const int C = p.C;
  const Lanes L = make_lanes(C);
  if (!L.active) return;
  const f32x4 sc = ld4(p.coef + 2 * C + 4 * L.cq), sh = ld4(p.coef + 3 * C + 4 * L.cq);
  for (long pix = (long)local * L.P + L.pl; pix < p.npix; pix += (long)nblk * L.P) {
    f32x4 v = bn_affine(ld4(p.y + pix * p.ldy + 4 * L.cq), sc, sh);
    if (p.residual) {       // (residual_split: the block input is stored pre-split for its convolution readers; hi + lo is its value)
      const float* r = p.residual + pix * p.ldr + 4 * L.cq;
      v += p.residual_split ? hrseg_join_f16x2(*reinterpret_cast<const u32x4*>(r)) : ld4(r);
    }
    if (p.relu) {
      // one byte per (pixel, channel quad): bit j = "channel 4q+j passed the ReLU".  With a residual the backward cannot
      // recompute the mask from y alone; reading this byte instead of z saves it 4 B per element, twice
      if (p.relu_mask) p.relu_mask[pix * L.Q + L.cq] = (unsigned char)((v[0] > 0.f) | ((v[1] > 0.f) << 1) | ((v[2] > 0.f) << 2) | ((v[3] > 0.f) << 3));
      v = relu_nan(v);       // (a NaN element's mask bit is 0: its gradient is masked, the value itself stays loud)
    }
    // z_split: the tensor's only readers are fp16x2 convolutions that take their pixel operand pre-split (hrseg_conv_shape_t.
    // x_split): the granule goes out as {hi01, hi23, lo01, lo23} -- the same 16 bytes per 4 channels, the split done once here
    // (a bandwidth-bound kernel with VALU to spare) instead of by every staging wave of the readers
    if (p.z_split) *reinterpret_cast<u32x4*>(p.z + pix * p.ldz + 4 * L.cq) = hrseg_split_f16x2(v);
    else st4(p.z + pix * p.ldz + 4 * L.cq, v);
  }
}

// MASK = some problem of the launch brings ReLU mask bytes.  Two instances because of REGISTERS: beside the 64-channel
// nine-tap weight gradient of the side stream (394 registers per lane of a SIMD) a wave of this kernel only fits under 112;
// the mask path costs 11 more (118) -- with one instance the UNet step, which has no masked layer at all, lost 2 ms of overlap.
template <bool MASK>
__global__ __launch_bounds__(256) void bn_bwd_reduce_group_kernel(BnBwdG g) {
  __shared__ double red[256 * 8];
  int local, nblk;
  const hrseg_bn_bwd_t& p = g.p[bn_find(g.h, local, nblk)];
  const int nseg = p.nseg > 1 ? p.nseg : 1;
  // the |dy| slots the apply kernel raises with atomicMax start from zero: reset here, two launches earlier on the stream
  if (local == 0 && threadIdx.x < 64 && p.dy_absmax) p.dy_absmax[threadIdx.x] = 0.f;
  stats_body<MASK>(p.dz, p.lddz, p.z, p.ldz, p.relu, p.y, p.ldy, p.coef, p.npix, p.C, p.partial, local, p.nchunks, true, red,
                   nseg, p.relu_mask);
}

__global__ __launch_bounds__(256) void bn_bwd_finalize_group_kernel(BnBwdG g) {
  __shared__ double red[512];
  int local, nblk;
  const hrseg_bn_bwd_t& p = g.p[bn_find(g.h, local, nblk)];
  const int C = p.C, c = local * 16 + (threadIdx.x & 15);
  const int nseg = p.nseg > 1 ? p.nseg : 1, cps = p.nchunks / nseg;
  double* totals = p.partial + (size_t)p.nchunks * 2 * C;      // [nseg][2][C]
  double s_all = 0.0, sx_all = 0.0;
  for (int seg = 0; seg < nseg; ++seg) {
    double s, sx;
    if (seg) __syncthreads();                                   // red is reused
    reduce_chunks16(p.partial + (size_t)seg * cps * 2 * C, cps, C, c, s, sx, red);
    if (threadIdx.x < 16 && c < C) {
      if (p.sum_ranks > 1) {               // sums over all ranks -> this rank's share (means stay global: the apply divides by the local count)
        s /= (double)p.sum_ranks;
        sx /= (double)p.sum_ranks;
      }
      totals[(size_t)seg * 2 * C + c] = s;
      totals[(size_t)seg * 2 * C + C + c] = sx;
      s_all += s;
      sx_all += sx;
    }
  }
  if (threadIdx.x >= 16 || c >= C) return;
  if (p.dgamma) p.dgamma[c] += (float)sx_all;
  if (p.dbeta) p.dbeta[c] += (float)s_all;
}

__global__ __launch_bounds__(256) void bn_bwd_apply_group_kernel(BnBwdG g, int eval_mode) {
  int local, nblk;
  const hrseg_bn_bwd_t& p = g.p[bn_find(g.h, local, nblk)];
  const int C = p.C;
  const Lanes L = make_lanes(C);
  float amax = 0.f;
  if (L.active) {                 // (no early return: every lane takes part in the max reduction below)
  const double* totals = p.partial + (size_t)p.nchunks * 2 * C;
  const f32x4 mean = ld4(p.coef + 4 * L.cq), rstd = ld4(p.coef + C + 4 * L.cq), scale = ld4(p.coef + 2 * C + 4 * L.cq);
  const f32x4 shift = ld4(p.coef + 3 * C + 4 * L.cq);
  const int nseg = p.nseg > 1 ? p.nseg : 1;
  const long seg_pix = p.npix / nseg;
  const float inv = eval_mode ? 0.f : (float)(1.0 / (double)seg_pix);
  for (int seg = 0; seg < nseg; ++seg) {
  f32x4 mg, mgx;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    mg[j] = (float)(totals[(size_t)seg * 2 * C + 4 * L.cq + j]) * inv;
    mgx[j] = (float)(totals[(size_t)seg * 2 * C + C + 4 * L.cq + j]) * inv;
  }
  for (long pix = seg * seg_pix + (long)local * L.P + L.pl; pix < (seg + 1) * seg_pix; pix += (long)nblk * L.P) {
    f32x4 gg = ld4(p.dz + pix * p.lddz + 4 * L.cq);
    const f32x4 yv = ld4(p.y + pix * p.ldy + 4 * L.cq);
    if (p.relu && p.relu_mask) {
      const unsigned bm = p.relu_mask[pix * L.Q + L.cq];
#pragma unroll
      for (int j = 0; j < 4; ++j) gg[j] = ((bm >> j) & 1u) ? gg[j] : 0.f;
    } else if (p.relu) {
      const f32x4 zz = p.z ? ld4(p.z + pix * p.ldz + 4 * L.cq) : bn_affine(yv, scale, shift);
#pragma unroll
      for (int j = 0; j < 4; ++j) gg[j] = zz[j] > 0.f ? gg[j] : 0.f;
    }
    const f32x4 xh = (yv - mean) * rstd;
    const f32x4 dyv = scale * (gg - mg - xh * mgx);
    st4(p.dy + pix * p.lddy + 4 * L.cq, dyv);
#pragma unroll
    for (int j = 0; j < 4; ++j) amax = fmaxf(amax, abs_nan_inf(dyv[j]));
    if (p.dres) {
      float* d = p.dres + pix * p.lddres + 4 * L.cq;
      st4(d, p.dres_accumulate ? ld4(d) + gg : gg);
    }
  }
  }
  }
  if (p.dy_absmax) {
    // max|dy| of the tensor into slot (block % 64) of a 64-entry array (non-negative floats order like their bit
    // patterns): one atomic per block, at most grid/64 per address -- a single address serialises ~4000 blocks
    __shared__ float wmax[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = amax;
    __syncthreads();
    if (threadIdx.x == 0) {
      const float m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
      if (m > 0.f) atomicMax(reinterpret_cast<unsigned*>(p.dy_absmax) + (blockIdx.x & 63), __float_as_uint(m));
    }
  }
}

// =========================================================================== level heads fused into the BatchNorm backward
// The layer in front of the level heads (HRNet shared head: conv -> BatchNorm -> ReLU, no residual, the heads its only readers):
// its normalised output f and the heads' feature gradient g are functions of y and of at most 8 logit-gradient values per pixel,
// so the backward runs as two passes over y (hrseg.h, hrseg_head_bn_t) instead of fill + head_bwd + reduce + apply over f / g.
//
// First pass = head_bwd_kernel's accumulations + stats_body's backward sums, on stats_body's chunks and in its per-thread pixel
// order (thread (cq, pl) walks lo + pl, lo + pl + P, ...; four pixels per trip), so the BatchNorm partials are the ones
// bn_bwd_reduce_group_kernel computes from the stored g.  A chunk may cross a sample boundary inside its segment: the FiLM pair
// and the dgb accumulators are per sample, so a thread flushes them (atomics) when its pixel sequence enters the next sample.
template <int CO>
__global__ __launch_bounds__(256) void head_bn_bwd_reduce_kernel(hrseg_head_bn_t a, int chunk0) {
  __shared__ double red[256 * 8];
  const int C = a.F;
  const Lanes L = make_lanes(C);
  const int chunk = chunk0 + blockIdx.x;
  const int cps = a.nchunks / a.nseg, seg = chunk / cps;
  const long hw = a.hw, seg_pix = (long)a.B * hw;
  const long per = (seg_pix + cps - 1) / cps;
  const long seg_base = seg * seg_pix;
  const long lo = seg_base + (long)(chunk - seg * cps) * per;
  const long seg_end = seg_base + seg_pix;
  const long hi = (lo + per < seg_end) ? lo + per : seg_end;
  // the |dy| slots the apply pass raises with atomicMax start from zero (as bn_bwd_reduce_group_kernel)
  if (blockIdx.x == 0 && threadIdx.x < 64 && a.dy_absmax) a.dy_absmax[threadIdx.x] = 0.f;
  const float* __restrict__ gb = a.gb[seg];
  const float* __restrict__ w = a.w[seg];
  const float* __restrict__ dzl = a.dzl[seg];
  const int lddz = a.lddzl[seg], Cout = a.Cout[seg];
  float* dgb = a.dgb[seg];
  f32x4 s = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
  f32x4 a_dw[CO], a_dg = {0.f, 0.f, 0.f, 0.f}, a_db = {0.f, 0.f, 0.f, 0.f};
  float a_bias[CO];
#pragma unroll
  for (int c = 0; c < CO; ++c) {
    a_dw[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    a_bias[c] = 0.f;
  }
  if (L.active && lo + L.pl < hi) {
    const f32x4 mean = ld4(a.coef + 4 * L.cq), rstd = ld4(a.coef + C + 4 * L.cq);
    const f32x4 sc = ld4(a.coef + 2 * C + 4 * L.cq), sh = ld4(a.coef + 3 * C + 4 * L.cq);
    f32x4 wq[CO];
#pragma unroll
    for (int c = 0; c < CO; ++c) wq[c] = (c < Cout) ? ld4(w + c * C + 4 * L.cq) : f32x4{0.f, 0.f, 0.f, 0.f};
    long b = (lo + L.pl - seg_base) / hw;           // sample of the thread's current pixel, bnd = first pixel of the next one
    long bnd = seg_base + (b + 1) * hw;
    f32x4 gam = {1.f, 1.f, 1.f, 1.f}, bet = {0.f, 0.f, 0.f, 0.f};
    if (gb) {
      gam = ld4(gb + (size_t)b * 2 * C + 4 * L.cq);
      bet = ld4(gb + (size_t)b * 2 * C + C + 4 * L.cq);
    }
    auto flush_dgb = [&]() {
      if (dgb) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          atomicAdd(dgb + (size_t)b * 2 * C + 4 * L.cq + j, a_dg[j]);
          atomicAdd(dgb + (size_t)b * 2 * C + C + 4 * L.cq + j, a_db[j]);
        }
      }
    };
    // pixels per trip, all loads issued before the first use.  The launch has one block per chunk (a wave per SIMD at 256 chunks),
    // and unlike stats_body only ONE 16-byte stream per pixel: eight pixels in flight where the registers allow it (the per-thread
    // order of the additions does not depend on U)
    constexpr int U = CO <= 4 ? 8 : 4;
    for (long pix0 = lo + L.pl; pix0 < hi; pix0 += (long)U * L.P) {
      f32x4 yv[U];
      float g[U][CO];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long pix = pix0 + (long)u * L.P;
        const bool ok = pix < hi;
        yv[u] = ok ? ld4(a.y + pix * a.ldy + 4 * L.cq) : mean;
#pragma unroll
        for (int c = 0; c < CO; ++c) g[u][c] = (ok && c < Cout) ? dzl[(pix - seg_base) * lddz + c] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long pix = pix0 + (long)u * L.P;
        if (pix >= hi) break;
        while (pix >= bnd) {                        // the sequence entered the next sample: its FiLM pair, its dgb rows
          flush_dgb();
          a_dg = f32x4{0.f, 0.f, 0.f, 0.f};
          a_db = f32x4{0.f, 0.f, 0.f, 0.f};
          ++b;
          bnd += hw;
          if (gb) {
            gam = ld4(gb + (size_t)b * 2 * C + 4 * L.cq);
            bet = ld4(gb + (size_t)b * 2 * C + C + 4 * L.cq);
          }
        }
        const f32x4 zc = bn_affine(yv[u], sc, sh);
        const f32x4 fv = relu_nan(zc);
        // head_bwd_kernel's `one`, with f recomputed
        const f32x4 fm = fv * gam + bet;
        f32x4 uu = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < CO; ++c) {
          uu += wq[c] * g[u][c];
          a_dw[c] += fm * g[u][c];
          if (L.cq == 0) a_bias[c] += g[u][c];
        }
        a_dg += fv * uu;
        a_db += uu;
        // stats_body's backward sums of the gradient head_bwd_kernel would have stored (gam * u), masked by the ReLU
        f32x4 gv = gam * uu;
#pragma unroll
        for (int j = 0; j < 4; ++j) gv[j] = zc[j] > 0.f ? gv[j] : 0.f;
        const f32x4 xh = (yv[u] - mean) * rstd;
        s += gv;
        s2 += gv * xh;
      }
    }
    flush_dgb();
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    red[threadIdx.x * 8 + j] = s[j];
    red[threadIdx.x * 8 + 4 + j] = s2[j];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    double sa = 0.0, sb = 0.0;
    for (int pl = 0; pl < L.P; ++pl) {
      const int t = pl * L.Q + (c >> 2);
      sa += red[t * 8 + (c & 3)];
      sb += red[t * 8 + 4 + (c & 3)];
    }
    a.partial[((size_t)chunk * 2 + 0) * C + c] = sa;
    a.partial[((size_t)chunk * 2 + 1) * C + c] = sb;
  }
  // dW / dbias: reduce over the pixel lanes of the block, then one atomic per (channel, output) -- as head_bwd_kernel
  float* fred = reinterpret_cast<float*>(red);
  float* dw = a.dw[seg];
  float* dbias = a.dbias[seg];
  auto reduce_add = [&](float v, float* dst) {
    __syncthreads();
    fred[threadIdx.x] = v;
    __syncthreads();
    if (L.active && L.pl == 0) {
      float t = 0.f;
      for (int q = 0; q < L.P; ++q) t += fred[q * L.Q + L.cq];
      atomicAdd(dst, t);
    }
  };
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int c = 0; c < CO; ++c)
      if (c < Cout) reduce_add(a_dw[c][j], dw + c * C + 4 * (L.active ? L.cq : 0) + j);
  if (dbias) {
#pragma unroll
    for (int c = 0; c < CO; ++c)
      if (c < Cout) {
        __syncthreads();
        fred[threadIdx.x] = (L.active && L.cq == 0) ? a_bias[c] : 0.f;
        __syncthreads();
        if (threadIdx.x == 0) {
          float t = 0.f;
          for (int q = 0; q < L.P; ++q) t += fred[q * L.Q];
          atomicAdd(dbias + c, t);
        }
      }
  }
}

// The first pass for wide rows (more than 128 channel quads: P = 1, every working thread walks EVERY pixel of its chunk).  The
// kernel above keeps 8 x 16 bytes per thread in flight and stops loading while it adds: one wave per SIMD, 23 KB per block, and
// the launch has one block per chunk on half the chip.  Here the block has a second set of 256 threads that only move data: they
// stream the chunk's rows (and the rows' logit gradients) through registers into a two-slot ring in LDS, two stages of
// HEAD_RING_ROWS rows in flight beside the one being written, while the first 256 threads -- thread cq the sums of channel quad
// cq, as above -- take their 16 bytes per pixel from the ring.  The additions are the ones of the kernel above, per thread in the
// same order, with the sample-boundary flush at the same pixel: the partial sums and what goes into the atomics are the same bits.
// A block depends on nothing but its own loads; the stage barrier orders LDS traffic only (no vmcnt(0): conv_ws.hip).  Stages
// come in pairs (the loaders alternate two register sets, and a loop with one exit is what lets the compiler count their loads
// exactly): an odd count is rounded up, the extra stage holds no pixel.
#define HEAD_RING_ROWS 16
static size_t head_ring_lds_bytes(int F) { return (size_t)2 * HEAD_RING_ROWS * (F + 8) * sizeof(float); }
template <int CO>
__global__ __launch_bounds__(512) void head_bn_bwd_reduce_ring_kernel(hrseg_head_bn_t a, int chunk0) {
  extern __shared__ __attribute__((aligned(16))) float ring[];      // y rows [2][R][F], then logit gradients [2][R][8]
  constexpr int R = HEAD_RING_ROWS;
  const int C = a.F, Q = C >> 2;
  float* const ybuf = ring;
  float* const gbuf = ring + (size_t)2 * R * C;
  const bool loader = __builtin_amdgcn_readfirstlane((int)threadIdx.x) >= 256;      // wave-uniform: a scalar branch
  const int cq = threadIdx.x & 255;
  const bool active = cq < Q;
  const int chunk = chunk0 + blockIdx.x;
  const int cps = a.nchunks / a.nseg, seg = chunk / cps;
  const long hw = a.hw, seg_pix = (long)a.B * hw;
  const long per = (seg_pix + cps - 1) / cps;
  const long seg_base = seg * seg_pix;
  const long lo = seg_base + (long)(chunk - seg * cps) * per;
  const long seg_end = seg_base + seg_pix;
  const long hi = (lo + per < seg_end) ? lo + per : seg_end;
  const int nst = lo < hi ? (int)(((hi - lo + R - 1) / R + 1) & ~1L) : 0;
  if (blockIdx.x == 0 && threadIdx.x < 64 && a.dy_absmax) a.dy_absmax[threadIdx.x] = 0.f;
  const float* __restrict__ gb = a.gb[seg];
  const float* __restrict__ w = a.w[seg];
  const float* __restrict__ dzl = a.dzl[seg];
  const int lddz = a.lddzl[seg], Cout = a.Cout[seg];
  float* dgb = a.dgb[seg];
  auto stage_barrier = [&]() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  };
  if (loader) {
    // No branch around a load and none around a store: rows past the chunk's end re-read its last row, threads past the last
    // channel quad the last quad, every thread brings the logit gradients of row cq % R (equal bytes stored twice) -- so the
    // compiler counts the loads in flight exactly and waits for one stage's registers with the next stage's still outstanding.
    if (nst > 0) {
      const int lcq = active ? cq : Q - 1, gr = cq & (R - 1);
      f32x4 va[R], vb[R];
      float ga[CO], gv[CO];
      auto issue = [&](f32x4 (&v)[R], float (&g)[CO], int st) {
        const long p0 = lo + (long)st * R;
        asm volatile("" ::: "memory");
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const long pix = (p0 + r < hi) ? p0 + r : hi - 1;
          v[r] = ld4(a.y + pix * a.ldy + 4 * lcq);
        }
        const long gp = (p0 + gr < hi) ? p0 + gr : hi - 1;
#pragma unroll
        for (int c = 0; c < CO; ++c) g[c] = dzl[(gp - seg_base) * lddz + (c < Cout ? c : Cout - 1)];
        asm volatile("" ::: "memory");
      };
      auto write = [&](const f32x4 (&v)[R], const float (&g)[CO], int st) {
        float* ys = ybuf + (size_t)(st & 1) * R * C + 4 * lcq;
#pragma unroll
        for (int r = 0; r < R; ++r) st4(ys + r * C, v[r]);
        float* gs = gbuf + ((st & 1) * R + gr) * 8;
#pragma unroll
        for (int c = 0; c < CO; ++c) gs[c] = (c < Cout) ? g[c] : 0.f;
      };
      issue(va, ga, 0);
      issue(vb, gv, 1);
      write(va, ga, 0);
      issue(va, ga, 2);
      stage_barrier();
      // trip t: the consumers read stage t; stage t + 1 goes into the other slot (read last in trip t - 1), its registers
      // take stage t + 3
      for (int t = 0; t < nst; t += 2) {
        write(vb, gv, t + 1);
        issue(vb, gv, t + 3);
        stage_barrier();
        write(va, ga, t + 2);
        issue(va, ga, t + 4);
        stage_barrier();
      }
    }
    return;
  }
  f32x4 s = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
  f32x4 a_dw[CO], a_dg = {0.f, 0.f, 0.f, 0.f}, a_db = {0.f, 0.f, 0.f, 0.f};
  float a_bias[CO];
#pragma unroll
  for (int c = 0; c < CO; ++c) {
    a_dw[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    a_bias[c] = 0.f;
  }
  // dbias (the plain sum of the logit gradients over the chunk, the same chain of additions in any thread): the adding waves
  // are bound by their vector instructions, so where the fourth wave holds no channel quad (at most 192 of them) its first
  // thread keeps this sum and the other three waves skip its two instructions per pixel; otherwise thread 0 as above
  const int bias_tid = Q <= 192 ? 192 : 0;
  const bool bias_wave = (__builtin_amdgcn_readfirstlane((int)threadIdx.x) >> 6) == (bias_tid >> 6);
  float* dbias = a.dbias[seg];
  if (nst > 0) {
    const int ccq = active ? cq : 0;
    const f32x4 mean = ld4(a.coef + 4 * ccq), rstd = ld4(a.coef + C + 4 * ccq);
    const f32x4 sc = ld4(a.coef + 2 * C + 4 * ccq), sh = ld4(a.coef + 3 * C + 4 * ccq);
    f32x4 wq[CO];
#pragma unroll
    for (int c = 0; c < CO; ++c) wq[c] = (c < Cout) ? ld4(w + c * C + 4 * ccq) : f32x4{0.f, 0.f, 0.f, 0.f};
    long b = (lo - seg_base) / hw;                  // sample of the current pixel, bnd = first pixel of the next one
    long bnd = seg_base + (b + 1) * hw;
    f32x4 gam = {1.f, 1.f, 1.f, 1.f}, bet = {0.f, 0.f, 0.f, 0.f};
    if (gb) {
      gam = ld4(gb + (size_t)b * 2 * C + 4 * ccq);
      bet = ld4(gb + (size_t)b * 2 * C + C + 4 * ccq);
    }
    auto flush_dgb = [&]() {
      if (dgb && active) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          atomicAdd(dgb + (size_t)b * 2 * C + 4 * cq + j, a_dg[j]);
          atomicAdd(dgb + (size_t)b * 2 * C + C + 4 * cq + j, a_db[j]);
        }
      }
    };
    // one pixel: the expressions of head_bn_bwd_reduce_kernel, y and the logit gradients from the ring
    auto one = [&](auto with_bias, const float* ys, const float* gs) {
      const f32x4 yv = ld4(ys);
      float g[CO];
      const f32x4 g0 = ld4(gs);
#pragma unroll
      for (int c = 0; c < (CO < 4 ? CO : 4); ++c) g[c] = g0[c];
      if (CO > 4) {
        const f32x4 g1 = ld4(gs + 4);
#pragma unroll
        for (int c = 4; c < CO; ++c) g[c] = g1[c - 4];
      }
      const f32x4 zc = bn_affine(yv, sc, sh);
      const f32x4 fv = relu_nan(zc);
      const f32x4 fm = fv * gam + bet;
      f32x4 uu = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < CO; ++c) {
        uu += wq[c] * g[c];
        a_dw[c] += fm * g[c];
        if (decltype(with_bias)::value) a_bias[c] += g[c];
      }
      a_dg += fv * uu;
      a_db += uu;
      f32x4 gv = gam * uu;
#pragma unroll
      for (int j = 0; j < 4; ++j) gv[j] = zc[j] > 0.f ? gv[j] : 0.f;
      const f32x4 xh = (yv - mean) * rstd;
      s += gv;
      s2 += gv * xh;
    };
    auto stages = [&](auto with_bias) {
    stage_barrier();                                // stage 0 is in its slot
    for (int t = 0; t < nst; ++t) {
      const float* ys = ybuf + (size_t)(t & 1) * R * C + 4 * ccq;
      const float* gs = gbuf + (t & 1) * R * 8;
      const long p0 = lo + (long)t * R;
      if (p0 + R <= hi && p0 + R <= bnd) {          // a whole stage inside one sample
        constexpr int UR = CO <= 4 ? R : 4;         // (registers: the eight-output instance holds twice the accumulators)
#pragma unroll 1
        for (int r0 = 0; r0 < R; r0 += UR)
#pragma unroll
          for (int r = r0; r < r0 + UR; ++r) one(with_bias, ys + r * C, gs + r * 8);
      } else {
        for (int r = 0; r < R && p0 + r < hi; ++r) {
          while (p0 + r >= bnd) {                   // the sequence entered the next sample: its FiLM pair, its dgb rows
            flush_dgb();
            a_dg = f32x4{0.f, 0.f, 0.f, 0.f};
            a_db = f32x4{0.f, 0.f, 0.f, 0.f};
            ++b;
            bnd += hw;
            if (gb) {
              gam = ld4(gb + (size_t)b * 2 * C + 4 * ccq);
              bet = ld4(gb + (size_t)b * 2 * C + C + 4 * ccq);
            }
          }
          one(with_bias, ys + r * C, gs + r * 8);
        }
      }
      stage_barrier();
    }
    };
    if (bias_wave) stages(std::true_type());
    else stages(std::false_type());
    flush_dgb();
  }
  if (dbias && (int)threadIdx.x == bias_tid) {
#pragma unroll
    for (int c = 0; c < CO; ++c)
      if (c < Cout) {
        float t = 0.f;
        t += a_bias[c];
        atomicAdd(dbias + c, t);
      }
  }
  if (!active) return;
  // one pixel lane: the fp64 sum over lanes of the kernel above is 0.0 + the lane's value, the dW / dbias lane sums 0.f + it
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double sa = 0.0, sb = 0.0;
    sa += (double)s[j];
    sb += (double)s2[j];
    a.partial[((size_t)chunk * 2 + 0) * C + 4 * cq + j] = sa;
    a.partial[((size_t)chunk * 2 + 1) * C + 4 * cq + j] = sb;
  }
  float* dw = a.dw[seg];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int c = 0; c < CO; ++c)
      if (c < Cout) {
        float t = 0.f;
        t += a_dw[c][j];
        atomicAdd(dw + c * C + 4 * cq + j, t);
      }
}

// Second pass: bn_bwd_apply_group_kernel with g recomputed from y and the logit gradient instead of read from memory.
template <int CO>
__global__ __launch_bounds__(256) void head_bn_bwd_apply_kernel(hrseg_head_bn_t a) {
  const int C = a.F;
  const Lanes L = make_lanes(C);
  float amax = 0.f;
  if (L.active) {                 // (no early return: every lane takes part in the max reduction below)
    const double* totals = a.partial + (size_t)a.nchunks * 2 * C;
    const f32x4 mean = ld4(a.coef + 4 * L.cq), rstd = ld4(a.coef + C + 4 * L.cq), scale = ld4(a.coef + 2 * C + 4 * L.cq);
    const f32x4 shift = ld4(a.coef + 3 * C + 4 * L.cq);
    const long hw = a.hw, seg_pix = (long)a.B * hw;
    const float inv = (float)(1.0 / (double)seg_pix);
    for (int seg = 0; seg < a.nseg; ++seg) {
      f32x4 mg, mgx;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        mg[j] = (float)(totals[(size_t)seg * 2 * C + 4 * L.cq + j]) * inv;
        mgx[j] = (float)(totals[(size_t)seg * 2 * C + C + 4 * L.cq + j]) * inv;
      }
      const float* __restrict__ gb = a.gb[seg];
      const float* __restrict__ w = a.w[seg];
      const float* __restrict__ dzl = a.dzl[seg];
      const int lddz = a.lddzl[seg], Cout = a.Cout[seg];
      f32x4 wq[CO];
#pragma unroll
      for (int c = 0; c < CO; ++c) wq[c] = (c < Cout) ? ld4(w + c * C + 4 * L.cq) : f32x4{0.f, 0.f, 0.f, 0.f};
      for (int b = 0; b < a.B; ++b) {
        const f32x4 gam = gb ? ld4(gb + (size_t)b * 2 * C + 4 * L.cq) : f32x4{1.f, 1.f, 1.f, 1.f};
        const long r0 = (long)b * hw, r1 = r0 + hw;           // rows of this sample inside its segment
        for (long r = r0 + (long)blockIdx.x * L.P + L.pl; r < r1; r += (long)gridDim.x * L.P) {
          const long pix = seg * seg_pix + r;
          const f32x4 yv = ld4(a.y + pix * a.ldy + 4 * L.cq);
          f32x4 uu = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int c = 0; c < CO; ++c) uu += wq[c] * ((c < Cout) ? dzl[r * lddz + c] : 0.f);
          f32x4 gg = gam * uu;
          const f32x4 zz = bn_affine(yv, scale, shift);
#pragma unroll
          for (int j = 0; j < 4; ++j) gg[j] = zz[j] > 0.f ? gg[j] : 0.f;
          const f32x4 xh = (yv - mean) * rstd;
          const f32x4 dyv = scale * (gg - mg - xh * mgx);
          st4(a.dy + pix * a.lddy + 4 * L.cq, dyv);
#pragma unroll
          for (int j = 0; j < 4; ++j) amax = fmaxf(amax, abs_nan_inf(dyv[j]));
        }
      }
    }
  }
  if (a.dy_absmax) {
    __shared__ float wmax[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = amax;
    __syncthreads();
    if (threadIdx.x == 0) {
      const float m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
      if (m > 0.f) atomicMax(reinterpret_cast<unsigned*>(a.dy_absmax) + (blockIdx.x & 63), __float_as_uint(m));
    }
  }
}

// =========================================================================== C ABI
extern "C" int hrseg_bn_fold(const float* w, const float* bias, const float* gamma, const float* beta, const float* running_mean,
                             const float* running_var, float eps, int Cout, int row, float* w_out, float* b_out,
                             hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(w && running_mean && running_var && w_out && b_out && Cout > 0 && row > 0, "hrseg_bn_fold: bad arguments");
  hipLaunchKernelGGL(bn_fold_kernel, dim3(Cout), dim3(256), 0, (hipStream_t)stream, w, bias, gamma, beta, running_mean,
                     running_var, eps, row, w_out, b_out);
  HRSEG_LAUNCH_CHECK("bn_fold");
  return 0;
}

// what a problem must bring depends on the phases that run (bit 0 statistics, bit 1 finalize / eval coefficients, bit 2 apply)
static int check_bn_fwd(const hrseg_bn_fwd_t& p, int training, int phases) {
  if (int e = check_c(p.C, "hrseg_bn_fwd_group")) return e;
  const bool stats = training && (phases & 1), finalize = phases & 2, apply = phases & 4;
  HRSEG_CHECK_ARG(p.coef && al16(p.coef), "hrseg_bn_fwd_group: bad tensor arguments (coef)");
  HRSEG_CHECK_ARG(!(stats || apply) || (p.y && p.ldy >= p.C && p.ldy % 4 == 0 && al16(p.y)), "hrseg_bn_fwd_group: bad tensor arguments (y, ldy)");
  HRSEG_CHECK_ARG(!(stats || apply || (training && finalize)) || p.npix > 0, "hrseg_bn_fwd_group: bad tensor arguments (npix)");
  HRSEG_CHECK_ARG(!apply || (p.z && p.ldz >= p.C && p.ldz % 4 == 0 && al16(p.z)), "hrseg_bn_fwd_group: bad tensor arguments (the apply phase needs z, ldz)");
  if (apply && p.residual)
    if (int e = check_operand(p.residual, p.ldr, p.C, "hrseg_bn_fwd_group", "residual")) return e;
  HRSEG_CHECK_ARG(!(stats || (training && finalize)) || (p.partial && p.nchunks > 0), "hrseg_bn_fwd_group: training needs partial/nchunks");
  HRSEG_CHECK_ARG(training || !finalize || (p.running_mean && p.running_var), "hrseg_bn_fwd_group: eval needs running stats");
  return 0;
}

extern "C" int hrseg_bn_fwd_group(int n, const hrseg_bn_fwd_t* probs, int training, hrseg_stream_t stream) {
  return hrseg_bn_fwd_group_phases(n, probs, training, 7, stream);
}

extern "C" int hrseg_bn_fwd_group_phases(int n, const hrseg_bn_fwd_t* probs, int training, int phases, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(n >= 1 && n <= BN_MAXG && probs, "hrseg_bn_fwd_group: n must be 1..%d", BN_MAXG);
  HRSEG_CHECK_ARG(phases > 0 && phases <= 7, "hrseg_bn_fwd_group_phases: phases is a mask of bits 0..2");
  hipStream_t st = (hipStream_t)stream;
  BnFwdG g;
  g.h.n = n;
  for (int i = 0; i < n; ++i) {
    if (int e = check_bn_fwd(probs[i], training, phases)) return e;
    g.p[i] = probs[i];
  }
  int end = 0;
  if (training) {
    if (phases & 1) {
      for (int i = 0; i < n; ++i) { end += probs[i].nchunks; g.h.blk_end[i] = end; }
      hipLaunchKernelGGL(bn_stats_group_kernel, dim3(end), dim3(256), 0, st, g);
      HRSEG_LAUNCH_CHECK("bn_stats_group");
    }
    if (phases & 2) {
      end = 0;
      for (int i = 0; i < n; ++i) { end += ceil_div(probs[i].C, 16); g.h.blk_end[i] = end; }
      hipLaunchKernelGGL(bn_finalize_group_kernel, dim3(end), dim3(256), 0, st, g);
      HRSEG_LAUNCH_CHECK("bn_finalize_group");
    }
  } else if (phases & 2) {
    for (int i = 0; i < n; ++i) { end += ceil_div(probs[i].C, 64); g.h.blk_end[i] = end; }
    hipLaunchKernelGGL(bn_eval_coef_group_kernel, dim3(end), dim3(64), 0, st, g);
    HRSEG_LAUNCH_CHECK("bn_eval_coef_group");
  }
  if (phases & 4) {
    end = 0;
    for (int i = 0; i < n; ++i) { end += elem_grid(probs[i].npix, probs[i].C); g.h.blk_end[i] = end; }
    hipLaunchKernelGGL(bn_apply_group_kernel, dim3(end), dim3(256), 0, st, g);
    HRSEG_LAUNCH_CHECK("bn_apply_group");
  }
  return 0;
}

extern "C" int hrseg_bn_bwd_group(int n, const hrseg_bn_bwd_t* probs, int eval_mode, hrseg_stream_t stream) {
  return hrseg_bn_bwd_group_phases(n, probs, eval_mode, 7, stream);
}

extern "C" int hrseg_bn_bwd_group_phases(int n, const hrseg_bn_bwd_t* probs, int eval_mode, int phases, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(n >= 1 && n <= BN_MAXG && probs, "hrseg_bn_bwd_group: n must be 1..%d", BN_MAXG);
  HRSEG_CHECK_ARG(phases > 0 && phases <= 7, "hrseg_bn_bwd_group_phases: phases is a mask of bits 0..2");
  hipStream_t st = (hipStream_t)stream;
  BnBwdG g;
  g.h.n = n;
  for (int i = 0; i < n; ++i) {
    const hrseg_bn_bwd_t& p = probs[i];
    if (int e = check_c(p.C, "hrseg_bn_bwd_group")) return e;
    HRSEG_CHECK_ARG(p.dz && p.y && p.coef && p.dy && p.partial && p.npix > 0 && p.nchunks > 0,
                    "hrseg_bn_bwd_group: bad arguments");
    HRSEG_CHECK_ARG(p.nseg <= 1 || (p.nchunks % p.nseg == 0 && p.npix % p.nseg == 0),
                    "hrseg_bn_bwd_group: nseg=%d must divide nchunks=%d and npix", p.nseg, p.nchunks);
    if (int e = check_operand(p.dz, p.lddz, p.C, "hrseg_bn_bwd_group", "dz")) return e;
    if (int e = check_operand(p.y, p.ldy, p.C, "hrseg_bn_bwd_group", "y")) return e;
    if (int e = check_operand(p.dy, p.lddy, p.C, "hrseg_bn_bwd_group", "dy")) return e;
    if (p.relu && p.z)
      if (int e = check_operand(p.z, p.ldz, p.C, "hrseg_bn_bwd_group", "z")) return e;
    if (p.dres)
      if (int e = check_operand(p.dres, p.lddres, p.C, "hrseg_bn_bwd_group", "dres")) return e;
    HRSEG_CHECK_ARG(al16(p.coef), "hrseg_bn_bwd_group: coef must be 16-byte aligned");
    g.p[i] = p;
  }
  int end = 0;
  bool masked = false;
  for (int i = 0; i < n; ++i) masked = masked || (probs[i].relu && probs[i].relu_mask);
  if (phases & 1) {
    for (int i = 0; i < n; ++i) { end += probs[i].nchunks; g.h.blk_end[i] = end; }
    if (masked) hipLaunchKernelGGL(bn_bwd_reduce_group_kernel<true>, dim3(end), dim3(256), 0, st, g);
    else hipLaunchKernelGGL(bn_bwd_reduce_group_kernel<false>, dim3(end), dim3(256), 0, st, g);
    HRSEG_LAUNCH_CHECK("bn_bwd_reduce_group");
  }
  if (phases & 2) {
    end = 0;
    for (int i = 0; i < n; ++i) { end += ceil_div(probs[i].C, 16); g.h.blk_end[i] = end; }
    hipLaunchKernelGGL(bn_bwd_finalize_group_kernel, dim3(end), dim3(256), 0, st, g);
    HRSEG_LAUNCH_CHECK("bn_bwd_finalize_group");
  }
  if (phases & 4) {
    end = 0;
    for (int i = 0; i < n; ++i) { end += elem_grid(probs[i].npix, probs[i].C); g.h.blk_end[i] = end; }
    hipLaunchKernelGGL(bn_bwd_apply_group_kernel, dim3(end), dim3(256), 0, st, g, eval_mode);
    HRSEG_LAUNCH_CHECK("bn_bwd_apply_group");
  }
  return 0;
}

static int check_head_bn(const hrseg_head_bn_t* p, const char* who, int seg0, int nsegs) {
  HRSEG_CHECK_ARG(p, "%s: NULL problem", who);
  if (int e = check_c(p->F, who)) return e;
  HRSEG_CHECK_ARG(p->y && p->coef && p->partial && p->B > 0 && p->hw > 0 && p->nseg >= 1 && p->nseg <= HRSEG_HEAD_BN_MAX_SEG &&
                      p->nchunks > 0 && p->nchunks % p->nseg == 0 && p->ldy >= p->F && p->ldy % 4 == 0,
                  "%s: bad arguments (F=%d nseg=%d nchunks=%d ldy=%d)", who, p->F, p->nseg, p->nchunks, p->ldy);
  HRSEG_CHECK_ARG(seg0 >= 0 && nsegs >= 1 && seg0 + nsegs <= p->nseg, "%s: segments [%d, %d) of %d", who, seg0, seg0 + nsegs, p->nseg);
  for (int s = seg0; s < seg0 + nsegs; ++s) {
    HRSEG_CHECK_ARG(p->w[s] && p->dzl[s] && p->Cout[s] > 0 && p->Cout[s] <= 8 && p->lddzl[s] >= p->Cout[s],
                    "%s: segment %d: bad head (Cout=%d lddzl=%d)", who, s, p->Cout[s], p->lddzl[s]);
  }
  return 0;
}

extern "C" int hrseg_head_bn_bwd_reduce(const hrseg_head_bn_t* p, int seg0, int nsegs, hrseg_stream_t stream) {
  if (int e = check_head_bn(p, "hrseg_head_bn_bwd_reduce", seg0, nsegs)) return e;
  if (hrseg_g_deterministic) {
    hrseg_set_error("hrseg_head_bn_bwd_reduce: not offered in deterministic mode (atomic sums); use hrseg_head_bwd + hrseg_bn_bwd_group");
    return HRSEG_ERR_UNSUPPORTED;
  }
  int comax = 0;
  for (int s = seg0; s < seg0 + nsegs; ++s) {
    HRSEG_CHECK_ARG(p->dw[s] && (p->gb[s] == nullptr) == (p->dgb[s] == nullptr), "hrseg_head_bn_bwd_reduce: segment %d: dw is required, dgb goes with gb", s);
    comax = p->Cout[s] > comax ? p->Cout[s] : comax;
  }
  const int cps = p->nchunks / p->nseg;
  if (p->F / 4 > 128) {       // one pixel lane per block (P = 1): the ring kernel
    const size_t lds = head_ring_lds_bytes(p->F);
    static bool raised = false;         // dynamic LDS beyond 64 KB is asked for once per kernel
    if (!raised) {
      const int most = (int)head_ring_lds_bytes(1024);
      const hipError_t e4 = hipFuncSetAttribute(reinterpret_cast<const void*>(&head_bn_bwd_reduce_ring_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize, most);
      const hipError_t e8 = hipFuncSetAttribute(reinterpret_cast<const void*>(&head_bn_bwd_reduce_ring_kernel<8>), hipFuncAttributeMaxDynamicSharedMemorySize, most);
      if (e4 != hipSuccess || e8 != hipSuccess) {
        hrseg_set_error("hrseg_head_bn_bwd_reduce: %d bytes of LDS refused: %s", most, hipGetErrorString(e4 != hipSuccess ? e4 : e8));
        return HRSEG_ERR_LAUNCH;
      }
      raised = true;
    }
    if (comax <= 4) hipLaunchKernelGGL(head_bn_bwd_reduce_ring_kernel<4>, dim3(nsegs * cps), dim3(512), lds, (hipStream_t)stream, *p, seg0 * cps);
    else hipLaunchKernelGGL(head_bn_bwd_reduce_ring_kernel<8>, dim3(nsegs * cps), dim3(512), lds, (hipStream_t)stream, *p, seg0 * cps);
  } else if (comax <= 4) hipLaunchKernelGGL(head_bn_bwd_reduce_kernel<4>, dim3(nsegs * cps), dim3(256), 0, (hipStream_t)stream, *p, seg0 * cps);
  else hipLaunchKernelGGL(head_bn_bwd_reduce_kernel<8>, dim3(nsegs * cps), dim3(256), 0, (hipStream_t)stream, *p, seg0 * cps);
  HRSEG_LAUNCH_CHECK("head_bn_bwd_reduce");
  return 0;
}

extern "C" int hrseg_head_bn_bwd_apply(const hrseg_head_bn_t* p, hrseg_stream_t stream) {
  if (int e = check_head_bn(p, "hrseg_head_bn_bwd_apply", 0, p ? p->nseg : 1)) return e;
  HRSEG_CHECK_ARG(p->dy && p->lddy >= p->F && p->lddy % 4 == 0, "hrseg_head_bn_bwd_apply: bad dy (lddy=%d)", p->lddy);
  int comax = 0;
  for (int s = 0; s < p->nseg; ++s) comax = p->Cout[s] > comax ? p->Cout[s] : comax;
  const long npix = (long)p->nseg * p->B * p->hw;
  const int grid = elem_grid(npix, p->F);
  if (comax <= 4) hipLaunchKernelGGL(head_bn_bwd_apply_kernel<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, *p);
  else hipLaunchKernelGGL(head_bn_bwd_apply_kernel<8>, dim3(grid), dim3(256), 0, (hipStream_t)stream, *p);
  HRSEG_LAUNCH_CHECK("head_bn_bwd_apply");
  return 0;
}
