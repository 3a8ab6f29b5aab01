// The heads: global average pool and FiLM linear (the conditioning of a level on the level above), the 1x1 level heads
// forward and backward, and the resize of their low-resolution NHWC logits to full-resolution NCHW planes.  gfx950.
// Each family's kernels are followed by its entry points.  The FUSED head backward (hrseg_head_bn_bwd_reduce / _apply)
// is not here but in bn.hip: it is written on that unit's pixel chunking, whose partial sums it has to reproduce.
#include "common.h"
#include "level_common.h"

// --------------------------------------------------------------------------- GAP over NCHW planes
__global__ __launch_bounds__(256) void gap_partial_kernel(const float* __restrict__ p, double* __restrict__ part,
                                                          long hw, int nsplit) {
  __shared__ double red[4];
  const int row = blockIdx.y, sp = blockIdx.x;
  const long per = (hw + nsplit - 1) / nsplit;
  const long lo = sp * per, hi = (lo + per < hw) ? lo + per : hw;
  const float* r = p + (size_t)row * hw;
  float s = 0.f;
  for (long i = lo + threadIdx.x; i < hi; i += 256) s += r[i];
  double d = wave_sum_d((double)s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)row * nsplit + sp] = red[0] + red[1] + red[2] + red[3];
}
__global__ void gap_final_kernel(const double* __restrict__ part, float* __restrict__ cond, int rows, int nsplit,
                                 long hw) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  double s = 0.0;
  for (int i = 0; i < nsplit; ++i) s += part[(size_t)r * nsplit + i];
  cond[r] = (float)(s / (double)hw);
}

extern "C" int hrseg_gap_nchw(const float* p, float* cond, double* scratch, int BC, long hw, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(p && cond && scratch && BC > 0 && hw > 0, "hrseg_gap_nchw: bad arguments");
  const int nsplit = 64;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gap_partial_kernel, dim3(nsplit, BC), dim3(256), 0, st, p, scratch, hw, nsplit);
  HRSEG_LAUNCH_CHECK("gap_partial");
  hipLaunchKernelGGL(gap_final_kernel, dim3(ceil_div(BC, 64)), dim3(64), 0, st, scratch, cond, BC, nsplit, hw);
  HRSEG_LAUNCH_CHECK("gap_final");
  return 0;
}

// --------------------------------------------------------------------------- FiLM linear (tiny)
__global__ void film_linear_fwd_kernel(const float* cond, const float* wl, const float* bl, float* gb, int B, int Cc,
                                       int F2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * F2) return;
  const int b = i / F2, j = i - b * F2;
  float s = bl[j];
  for (int c = 0; c < Cc; ++c) s = fmaf(cond[b * Cc + c], wl[j * Cc + c], s);
  gb[i] = s;
}
// dcond[b][c] = scale * sum_j dgb[b][j] wl[j][c];  dwl[j][c] += sum_b dgb[b][j] cond[b][c];  dbl[j] += sum_b dgb[b][j]
__global__ void film_linear_bwd_kernel(const float* cond, const float* wl, const float* dgb, float* dcond, float* dwl,
                                       float* dbl, int B, int Cc, int F2, float scale) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < F2) {
    float sb = 0.f;
    for (int b = 0; b < B; ++b) sb += dgb[b * F2 + j];
    if (dbl) dbl[j] += sb;
    if (dwl)
      for (int c = 0; c < Cc; ++c) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s = fmaf(dgb[b * F2 + j], cond[b * Cc + c], s);
        dwl[j * Cc + c] += s;
      }
  }
  if (dcond && blockIdx.x == 0) {
    // one wave per output element, lanes stride the 2F-long dot product (one thread per element walked it alone:
    // 1440 dependent steps, 180 us for a 32-element result)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    for (int i = wave; i < B * Cc; i += nwave) {
      const int b = i / Cc, c = i - b * Cc;
      float s = 0.f;
      for (int jj = lane; jj < F2; jj += 64) s = fmaf(dgb[b * F2 + jj], wl[jj * Cc + c], s);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if (lane == 0) dcond[i] = s * scale;
    }
  }
}

extern "C" int hrseg_film_linear_fwd(const float* cond, const float* wl, const float* bl, float* gb, int B, int Cc,
                                     int F2, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(cond && wl && bl && gb && B > 0 && Cc > 0 && F2 > 0, "hrseg_film_linear_fwd: bad arguments");
  hipLaunchKernelGGL(film_linear_fwd_kernel, dim3(ceil_div((long)B * F2, 256)), dim3(256), 0, (hipStream_t)stream, cond,
                     wl, bl, gb, B, Cc, F2);
  HRSEG_LAUNCH_CHECK("film_linear_fwd");
  return 0;
}

extern "C" int hrseg_film_linear_bwd(const float* cond, const float* wl, const float* dgb, float* dcond, float* dwl,
                                     float* dbl, int B, int Cc, int F2, float dcond_scale, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(cond && wl && dgb && B > 0 && Cc > 0 && F2 > 0, "hrseg_film_linear_bwd: bad arguments");
  hipLaunchKernelGGL(film_linear_bwd_kernel, dim3(ceil_div(F2, 256)), dim3(256), 0, (hipStream_t)stream, cond, wl, dgb,
                     dcond, dwl, dbl, B, Cc, F2, dcond_scale);
  HRSEG_LAUNCH_CHECK("film_linear_bwd");
  return 0;
}

// --------------------------------------------------------------------------- head forward
// z[pix][c] = sum_k W[c][k] (f[pix][k] g[b][k] + be[b][k]) + bias[c].  Effective per-sample
// weights W*g and bias + W.be are built in LDS; LP lanes share one pixel row.
// BN: `f` is the un-normalised output y of the convolution in front of the BatchNorm + ReLU whose result the head reads, and
// `coef` that BatchNorm's [mean, rstd, scale, shift][F]: a feature is max(bn_affine(y, scale, shift), 0) on load -- the value
// bn_apply_group_kernel would have stored, so the logits are the same bits without the normalised tensor ever being written.
template <int LP, int CO, bool BN>
__global__ __launch_bounds__(256) void head_fwd_kernel(const float* __restrict__ f, int ldf,
                                                       const float* __restrict__ coef,
                                                       const float* __restrict__ gb, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ z, int ldz,
                                                       long hw, int F, int Cout) {
  extern __shared__ float sm[];  // weff[CO][F], beff[CO]
  float* weff = sm;
  float* beff = sm + CO * F;
  const int b = blockIdx.y;
  const float* gam = gb ? gb + (size_t)b * 2 * F : nullptr;
  for (int i = threadIdx.x; i < CO * F; i += 256) {
    const int c = i / F, k = i - c * F;
    weff[i] = (c < Cout) ? w[c * F + k] * (gam ? gam[k] : 1.f) : 0.f;
  }
  // beff[c] = bias[c] + sum_k w[c][k] * beta[k]: all 256 threads take part (four threads walking F elements each was
  // a 720-step serial chain at the head of every block: most of this kernel's time with FiLM on)
  {
    __shared__ float red[CO][4];
    float part[CO];
#pragma unroll
    for (int c = 0; c < CO; ++c) {
      part[c] = 0.f;
      if (gam && c < Cout)
        for (int k = threadIdx.x; k < F; k += 256) part[c] = fmaf(w[c * F + k], gam[F + k], part[c]);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) part[c] += __shfl_xor(part[c], o, 64);
      if ((threadIdx.x & 63) == 0) red[c][threadIdx.x >> 6] = part[c];
    }
    __syncthreads();
    if (threadIdx.x < CO) {
      const int c = threadIdx.x;
      beff[c] = ((c < Cout && bias) ? bias[c] : 0.f) + ((red[c][0] + red[c][1]) + (red[c][2] + red[c][3]));
    }
  }
  __syncthreads();
  constexpr int PPB = 256 / LP;  // pixels per block iteration
  const int sub = threadIdx.x % LP, pg = threadIdx.x / LP;
  const int Q = F >> 2;
  if (Q <= 3 * LP) {
    // a lane reads the same (at most three) 4-channel groups of every pixel: its slice of the effective weights lives
    // in registers for the whole block, and the pixel loop is global loads + FMAs only (reading the weights from LDS
    // per pixel was four ds_read_b128 per 16 bytes of features: 217 us for the 553 MB of the HRNet feature map)
    f32x4 wr[3][CO];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int c = 0; c < CO; ++c) {
        const int q = sub + j * LP;
        wr[j][c] = (q < Q) ? *reinterpret_cast<const f32x4*>(weff + c * F + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    f32x4 bsc[3], bsh[3];       // BN: scale / shift of the lane's channel groups (zero beyond Q: max(fma(0, 0, 0), 0) = 0)
    if (BN) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int q = sub + j * LP;
        bsc[j] = (q < Q) ? *reinterpret_cast<const f32x4*>(coef + 2 * F + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
        bsh[j] = (q < Q) ? *reinterpret_cast<const f32x4*>(coef + 3 * F + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    for (long pix = (long)blockIdx.x * PPB + pg; pix < hw; pix += (long)gridDim.x * PPB) {
      const float* row = f + ((size_t)b * hw + pix) * ldf;
      f32x4 v[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int q = sub + j * LP;
        v[j] = (q < Q) ? *reinterpret_cast<const f32x4*>(row + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
      if (BN) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          v[j] = relu_nan(bn_affine(v[j], bsc[j], bsh[j]));
        }
      }
      float acc[CO];
#pragma unroll
      for (int c = 0; c < CO; ++c) {
        acc[c] = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[c] += v[j][0] * wr[j][c][0] + v[j][1] * wr[j][c][1] + v[j][2] * wr[j][c][2] + v[j][3] * wr[j][c][3];
      }
#pragma unroll
      for (int c = 0; c < CO; ++c)
#pragma unroll
        for (int o = LP / 2; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o, 64);
      if (sub == 0) {
        float* o = z + ((size_t)b * hw + pix) * ldz;
#pragma unroll
        for (int c = 0; c < CO; ++c)
          if (c < Cout) o[c] = acc[c] + beff[c];
      }
    }
    return;
  }
  for (long pix = (long)blockIdx.x * PPB + pg; pix < hw; pix += (long)gridDim.x * PPB) {
    const float* row = f + ((size_t)b * hw + pix) * ldf;
    float acc[CO];
#pragma unroll
    for (int c = 0; c < CO; ++c) acc[c] = 0.f;
    for (int q = sub; q < Q; q += LP) {
      f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * q);
      if (BN) {
        v = relu_nan(bn_affine(v, *reinterpret_cast<const f32x4*>(coef + 2 * F + 4 * q), *reinterpret_cast<const f32x4*>(coef + 3 * F + 4 * q)));
      }
#pragma unroll
      for (int c = 0; c < CO; ++c) {
        const f32x4 ww = *reinterpret_cast<const f32x4*>(weff + c * F + 4 * q);
        acc[c] += v[0] * ww[0] + v[1] * ww[1] + v[2] * ww[2] + v[3] * ww[3];
      }
    }
#pragma unroll
    for (int c = 0; c < CO; ++c)
#pragma unroll
      for (int o = LP / 2; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o, 64);
    if (sub == 0) {
      float* o = z + ((size_t)b * hw + pix) * ldz;
#pragma unroll
      for (int c = 0; c < CO; ++c)
        if (c < Cout) o[c] = acc[c] + beff[c];
    }
  }
}

// head backward: thread owns channel quad cq of pixel lane pl; block = (pixel chunk, sample)
template <int CO>
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ f, int ldf,
                                                       const float* __restrict__ gb, const float* __restrict__ w,
                                                       const float* __restrict__ dz, int lddz,
                                                       float* __restrict__ df, int lddf, int df_acc,
                                                       float* __restrict__ dw, float* __restrict__ dbias,
                                                       float* __restrict__ dgb, long hw, int F, int Cout,
                                                       long pix_per_block, int b0) {
  __shared__ float red[256];
  const int Q = F >> 2;
  const int P = (Q >= 256) ? 1 : 256 / Q;
  const int cq = threadIdx.x % Q, pl = threadIdx.x / Q;
  const bool active = pl < P;
  const int b = blockIdx.y + b0;
  const long lo = (long)blockIdx.x * pix_per_block;
  const long hi = (lo + pix_per_block < hw) ? lo + pix_per_block : hw;
  f32x4 gam = {1.f, 1.f, 1.f, 1.f}, bet = {0.f, 0.f, 0.f, 0.f};
  f32x4 wq[CO];
  f32x4 a_dw[CO], a_dg = {0.f, 0.f, 0.f, 0.f}, a_db = {0.f, 0.f, 0.f, 0.f};
  float a_bias[CO];
#pragma unroll
  for (int c = 0; c < CO; ++c) {
    wq[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    a_dw[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    a_bias[c] = 0.f;
  }
  if (active) {
    if (gb) {
      gam = *reinterpret_cast<const f32x4*>(gb + (size_t)b * 2 * F + 4 * cq);
      bet = *reinterpret_cast<const f32x4*>(gb + (size_t)b * 2 * F + F + 4 * cq);
    }
#pragma unroll
    for (int c = 0; c < CO; ++c)
      if (c < Cout) wq[c] = *reinterpret_cast<const f32x4*>(w + c * F + 4 * cq);
    // four pixels per iteration, every load of the four before the arithmetic: with one channel group per thread and
    // one pixel per iteration the loop had a single 16-byte load in flight per thread
    constexpr int U = 4;
    auto one = [&](const f32x4& fv, const float (&g)[CO], const f32x4& dold, size_t r) {
      const f32x4 fm = fv * gam + bet;
      f32x4 u = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < CO; ++c) {
        u += wq[c] * g[c];
        a_dw[c] += fm * g[c];
        if (cq == 0) a_bias[c] += g[c];
      }
      a_dg += fv * u;
      a_db += u;
      if (df) *reinterpret_cast<f32x4*>(df + r * lddf + 4 * cq) = dold + gam * u;
    };
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const bool racc = df && df_acc;
    long pix = lo + pl;
    for (; pix + (long)(U - 1) * P < hi; pix += (long)U * P) {
      f32x4 fv[U], dold[U];
      float g[U][CO];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const size_t r = (size_t)b * hw + pix + (long)i * P;
        fv[i] = *reinterpret_cast<const f32x4*>(f + r * ldf + 4 * cq);
        dold[i] = racc ? *reinterpret_cast<const f32x4*>(df + r * lddf + 4 * cq) : zero;
#pragma unroll
        for (int c = 0; c < CO; ++c) g[i][c] = (c < Cout) ? dz[r * lddz + c] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < U; ++i) one(fv[i], g[i], dold[i], (size_t)b * hw + pix + (long)i * P);
    }
    for (; pix < hi; pix += P) {
      const size_t r = (size_t)b * hw + pix;
      float g[CO];
#pragma unroll
      for (int c = 0; c < CO; ++c) g[c] = (c < Cout) ? dz[r * lddz + c] : 0.f;
      one(*reinterpret_cast<const f32x4*>(f + r * ldf + 4 * cq), g, racc ? *reinterpret_cast<const f32x4*>(df + r * lddf + 4 * cq) : zero, r);
    }
  }
  // reduce over the pixel lanes of the block, then one atomic per (channel, output)
  auto reduce_add = [&](float v, float* dst) {
    red[threadIdx.x] = v;
    __syncthreads();
    if (active && pl == 0) {
      float s = 0.f;
      for (int q = 0; q < P; ++q) s += red[q * Q + cq];
      atomicAdd(dst, s);
    }
    __syncthreads();
  };
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int c = 0; c < CO; ++c)
      if (c < Cout) reduce_add(a_dw[c][j], dw + c * F + 4 * cq + j);
    if (dgb) {
      reduce_add(a_dg[j], dgb + (size_t)b * 2 * F + 4 * cq + j);
      reduce_add(a_db[j], dgb + (size_t)b * 2 * F + F + 4 * cq + j);
    }
  }
  if (dbias) {
#pragma unroll
    for (int c = 0; c < CO; ++c)
      if (c < Cout) {
        red[threadIdx.x] = (active && cq == 0) ? a_bias[c] : 0.f;
        __syncthreads();
        if (threadIdx.x == 0) {
          float s = 0.f;
          for (int q = 0; q < P; ++q) s += red[q * Q];
          atomicAdd(dbias + c, s);
        }
        __syncthreads();
      }
  }
}

static int head_fwd_launch(const char* who, const float* f, int ldf, const float* coef, const float* gb, const float* w,
                           const float* bias, float* z, int ldz, int B, long hw, int F, int Cout, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(f && w && z && B > 0 && hw > 0 && F > 0 && F % 4 == 0 && Cout > 0 && Cout <= 8 && ldf >= F &&
                      ldf % 4 == 0 && ldz >= Cout,
                  "%s: bad arguments (F=%d Cout=%d)", who, F, Cout);
  hipStream_t st = (hipStream_t)stream;
  const int co = Cout <= 4 ? 4 : 8;
  const size_t smem = (size_t)(co * F + co) * sizeof(float);
  const int lp = (F / 4 <= 16) ? 16 : 64;
  long blocks = (hw + (256 / lp) - 1) / (256 / lp);
  const long cap = (2048 + B - 1) / B < 64 ? 64 : (2048 + B - 1) / B;      // ~2048 blocks in all: the per-block set-up is paid once per CU slot
  if (blocks > cap) blocks = cap;
  dim3 grid((int)blocks, B);
#define HF(LP_, CO_)                                                                                                              \
  do {                                                                                                                            \
    if (coef) hipLaunchKernelGGL((head_fwd_kernel<LP_, CO_, true>), grid, dim3(256), smem, st, f, ldf, coef, gb, w, bias, z, ldz, \
                                 hw, F, Cout);                                                                                    \
    else hipLaunchKernelGGL((head_fwd_kernel<LP_, CO_, false>), grid, dim3(256), smem, st, f, ldf, coef, gb, w, bias, z, ldz, hw, \
                            F, Cout);                                                                                             \
  } while (0)
  if (lp == 16 && co == 4) HF(16, 4);
  else if (lp == 16) HF(16, 8);
  else if (co == 4) HF(64, 4);
  else HF(64, 8);
#undef HF
  HRSEG_LAUNCH_CHECK(who);
  return 0;
}

extern "C" int hrseg_head_fwd(const float* f, int ldf, const float* gb, const float* w, const float* bias, float* z,
                              int ldz, int B, long hw, int F, int Cout, hrseg_stream_t stream) {
  return head_fwd_launch("hrseg_head_fwd", f, ldf, nullptr, gb, w, bias, z, ldz, B, hw, F, Cout, stream);
}

extern "C" int hrseg_head_bn_fwd(const float* y, int ldy, const float* coef, const float* gb, const float* w, const float* bias,
                                 float* z, int ldz, int B, long hw, int F, int Cout, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(coef, "hrseg_head_bn_fwd: coef is required (hrseg_head_fwd reads a normalised tensor)");
  return head_fwd_launch("hrseg_head_bn_fwd", y, ldy, coef, gb, w, bias, z, ldz, B, hw, F, Cout, stream);
}

extern "C" int hrseg_head_bwd(const float* f, int ldf, const float* gb, const float* w, const float* dz, int lddz,
                              float* df, int lddf, int df_accumulate, float* dw, float* dbias, float* dgb, int B,
                              long hw, int F, int Cout, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(f && w && dz && dw && B > 0 && hw > 0 && F > 0 && F % 4 == 0 && F <= 1024 && Cout > 0 &&
                      Cout <= 8 && (gb == nullptr) == (dgb == nullptr),
                  "hrseg_head_bwd: bad arguments (F=%d Cout=%d)", F, Cout);
  // the kernel moves 16 bytes at f + r*ldf + 4*cq and df + r*lddf + 4*cq: a row stride that is not a multiple of 4 floats
  // would be a misaligned access, one below the row length an overlap
  HRSEG_CHECK_ARG(ldf >= F && ldf % 4 == 0 && lddz >= Cout && (df == nullptr || (lddf >= F && lddf % 4 == 0)),
                  "hrseg_head_bwd: bad row strides (ldf=%d lddz=%d lddf=%d for F=%d Cout=%d)", ldf, lddz, lddf, F, Cout);
  hipStream_t st = (hipStream_t)stream;
  long chunks = 2048 / B;
  if (chunks < 1) chunks = 1;
  long ppb = (hw + chunks - 1) / chunks;
  if (ppb < 64) ppb = 64;
  // deterministic: one block per image, the images one launch after the other (a single adder per dW element at a time)
  const int nlaunch = hrseg_g_deterministic ? B : 1;
  if (hrseg_g_deterministic) ppb = hw;
  dim3 grid(ceil_div(hw, ppb), hrseg_g_deterministic ? 1 : B);
  for (int b0 = 0; b0 < nlaunch; ++b0) {
    if (Cout <= 4)
      hipLaunchKernelGGL((head_bwd_kernel<4>), grid, dim3(256), 0, st, f, ldf, gb, w, dz, lddz, df, lddf, df_accumulate,
                         dw, dbias, dgb, hw, F, Cout, ppb, b0);
    else
      hipLaunchKernelGGL((head_bwd_kernel<8>), grid, dim3(256), 0, st, f, ldf, gb, w, dz, lddz, df, lddf, df_accumulate,
                         dw, dbias, dgb, hw, F, Cout, ppb, b0);
  }
  HRSEG_LAUNCH_CHECK("head_bwd");
  return 0;
}

// --------------------------------------------------------------------------- logits resize NHWC(low) -> NCHW(full)
__device__ __forceinline__ void src_index_ac(int o, float scale, int in_size, int align, int& i0, int& i1, float& l0,
                                             float& l1) {
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
__global__ void logits_up_fwd_kernel(const float* __restrict__ in, int ldin, int B, int Hi, int Wi, int C,
                                     float* __restrict__ out, int Ho, int Wo, float sh, float sw, int align) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long hw = (long)Ho * Wo;
  if (i >= B * hw) return;
  const int b = (int)(i / hw);
  const long p = i - b * hw;
  const int oy = (int)(p / Wo), ox = (int)(p - (long)oy * Wo);
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
  src_index_ac(oy, sh, Hi, align, y0, y1, ly0, ly1);
  src_index_ac(ox, sw, Wi, align, x0, x1, lx0, lx1);
  const float* base = in + (size_t)b * Hi * Wi * ldin;
  for (int c = 0; c < C; ++c) {
    const float v00 = base[((size_t)y0 * Wi + x0) * ldin + c], v01 = base[((size_t)y0 * Wi + x1) * ldin + c];
    const float v10 = base[((size_t)y1 * Wi + x0) * ldin + c], v11 = base[((size_t)y1 * Wi + x1) * ldin + c];
    out[((size_t)b * C + c) * hw + p] = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
  }
}
// weight of output index o on input index i (either tap), as the forward applies it
__device__ __forceinline__ float tap_weight(int o, float scale, int in_size, int align, int i) {
  int i0, i1;
  float l0, l1;
  src_index_ac(o, scale, in_size, align, i0, i1, l0, l1);
  return (i0 == i ? l0 : 0.f) + (i1 == i ? l1 : 0.f);
}
// narrows [lo, hi] to its first and last output index with a non-zero weight on i (nothing left: lo > hi)
__device__ __forceinline__ void tap_range(int& lo, int& hi, float scale, int in_size, int align, int i) {
  while (lo <= hi && tap_weight(lo, scale, in_size, align, i) == 0.f) ++lo;
  while (hi > lo && tap_weight(hi, scale, in_size, align, i) == 0.f) --hi;
}
// din[b,iy,ix,c] = sum over the output pixels touching (iy,ix): ONE fmaf chain per element over (oy, ox) in row-major order,
// zero weights skipped.  One thread per (channel, b, iy, ix), the pixel fastest (a wave reads runs of an output row of one
// plane): C times the threads of a thread per pixel, which at 155 x 155 x 4 was 1.5 waves per CU walking 121 candidates each.
// The candidate ranges are narrowed to the contributing rows and columns once per thread, before the double loop.
__global__ void logits_up_bwd_kernel(const float* __restrict__ dout, int B, int Hi, int Wi, int C,
                                     float* __restrict__ din, int lddin, int Ho, int Wo, float sh, float sw,
                                     int align) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long npix = (long)B * Hi * Wi;
  if (i >= npix * C) return;
  const int c = (int)(i / npix);
  const long pix = i - (long)c * npix;
  const int b = (int)(pix / ((long)Hi * Wi));
  const int rem = (int)(pix - (long)b * Hi * Wi);
  const int iy = rem / Wi, ix = rem - iy * Wi;
  const long hw = (long)Ho * Wo;
  const float ish = sh > 0.f ? 1.f / sh : 0.f, isw = sw > 0.f ? 1.f / sw : 0.f;
  const float hf = align ? 0.f : 0.5f;
  int oy_lo = 0, oy_hi = Ho - 1, ox_lo = 0, ox_hi = Wo - 1;
  if (sh > 0.f) {
    oy_lo = max(0, (int)floorf(((float)iy - 1.f + hf) * ish - hf) - 1);
    oy_hi = min(Ho - 1, (int)ceilf(((float)iy + 1.f + hf) * ish - hf) + 1);
  }
  if (sw > 0.f) {
    ox_lo = max(0, (int)floorf(((float)ix - 1.f + hf) * isw - hf) - 1);
    ox_hi = min(Wo - 1, (int)ceilf(((float)ix + 1.f + hf) * isw - hf) + 1);
  }
  tap_range(oy_lo, oy_hi, sh, Hi, align, iy);
  tap_range(ox_lo, ox_hi, sw, Wi, align, ix);
  const float* __restrict__ plane = dout + ((size_t)b * C + c) * hw;
  float s = 0.f;
  for (int oy = oy_lo; oy <= oy_hi; ++oy) {
    const float wy = tap_weight(oy, sh, Hi, align, iy);
    if (wy == 0.f) continue;
    for (int ox = ox_lo; ox <= ox_hi; ++ox) {
      const float wx = tap_weight(ox, sw, Wi, align, ix);
      if (wx == 0.f) continue;
      const float wgt = wy * wx;
      s = fmaf(wgt, plane[(size_t)oy * Wo + ox], s);
    }
  }
  din[pix * lddin + c] = s;
}

static float up_scale(int in_size, int out_size, int align) {
  if (align) return out_size > 1 ? (float)(in_size - 1) / (float)(out_size - 1) : 0.f;
  return (float)in_size / (float)out_size;
}

extern "C" int hrseg_logits_up_fwd(const float* in, int ldin, int B, int Hi, int Wi, int C, float* out, int Ho, int Wo,
                                   int align_corners, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(in && out && B > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && C > 0 && C <= MAXC && ldin >= C,
                  "hrseg_logits_up_fwd: bad arguments");
  const long n = (long)B * Ho * Wo;
  hipLaunchKernelGGL(logits_up_fwd_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, in, ldin, B, Hi,
                     Wi, C, out, Ho, Wo, up_scale(Hi, Ho, align_corners), up_scale(Wi, Wo, align_corners),
                     align_corners);
  HRSEG_LAUNCH_CHECK("logits_up_fwd");
  return 0;
}

extern "C" int hrseg_logits_up_bwd(const float* dout, int B, int Hi, int Wi, int C, float* din, int lddin, int Ho,
                                   int Wo, int align_corners, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(dout && din && B > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && C > 0 && C <= MAXC && lddin >= C,
                  "hrseg_logits_up_bwd: bad arguments");
  const long n = (long)B * Hi * Wi;
  hipLaunchKernelGGL(logits_up_bwd_kernel, dim3(ceil_div(n * C, 128)), dim3(128), 0, (hipStream_t)stream, dout, B, Hi, Wi,
                     C, din, lddin, Ho, Wo, up_scale(Hi, Ho, align_corners), up_scale(Wi, Wo, align_corners),
                     align_corners);
  HRSEG_LAUNCH_CHECK("logits_up_bwd");
  return 0;
}
