// The per-level kernels templated on CT, the level's channel count rounded up to 4 / 8 / 16, and what hangs off them: the
// fused CE + soft-Dice loss (forward partials, finalize, gradient), the per-step prediction / confusion-count kernel and
// the metric vectors computed from its counts.  gfx950.  Each family's kernels are followed by its entry points.
//
// Logits / targets here are NCHW fp32 planes ([B,C,hw]) as the reference returns them; a thread owns one pixel and holds
// its CT channels in registers.
#include <cfloat>

#include "common.h"
#include "level_common.h"
#include "ohem.h"

// launches KERNEL<CT> (256-thread blocks, no dynamic LDS) with the smallest CT of 4 / 8 / 16 that holds C channels
#define LAUNCH_CT(KERNEL, C, grid, st, ...)                                                  \
  do {                                                                                       \
    if ((C) <= 4) hipLaunchKernelGGL((KERNEL<4>), grid, dim3(256), 0, st, __VA_ARGS__);      \
    else if ((C) <= 8) hipLaunchKernelGGL((KERNEL<8>), grid, dim3(256), 0, st, __VA_ARGS__); \
    else hipLaunchKernelGGL((KERNEL<16>), grid, dim3(256), 0, st, __VA_ARGS__);              \
  } while (0)

// the same ladder for kernels with three more template arguments: KERNEL<CT, FLAG, FLAG2, FLAG3>
#define LAUNCH_CT_FLAGS(KERNEL, FLAG, FLAG2, FLAG3, C, grid, st, ...)                                            \
  do {                                                                                                           \
    if ((C) <= 4) hipLaunchKernelGGL((KERNEL<4, FLAG, FLAG2, FLAG3>), grid, dim3(256), 0, st, __VA_ARGS__);      \
    else if ((C) <= 8) hipLaunchKernelGGL((KERNEL<8, FLAG, FLAG2, FLAG3>), grid, dim3(256), 0, st, __VA_ARGS__); \
    else hipLaunchKernelGGL((KERNEL<16, FLAG, FLAG2, FLAG3>), grid, dim3(256), 0, st, __VA_ARGS__);              \
  } while (0)

// --------------------------------------------------------------------------- loss
// Focal CE (the FOCAL instances, gamma > 0): the per-pixel term is -t (1-p)^gamma log p.  om = 1 - p_c arrives as the sum of
// the OTHER channels' exponentials over the softmax denominator, never as 1 - p: the subtraction is 0 in fp32 once a logit
// gap passes 17, and for gamma < 1 the gradient factor (1-p)^(gamma-1) then makes 0 * inf.  `rest` = the exponentials after
// channel c summed from the top (filled by focal_suffix), `pre` = those before it.
template <int CT>
__device__ __forceinline__ void focal_suffix(const float (&e)[CT], float (&rest)[CT]) {
  float r = 0.f;
#pragma unroll
  for (int c = CT - 1; c >= 0; --c) {
    rest[c] = r;
    r += e[c];
  }
}
// (1-p)^gamma; the limit at om -> 0 is 0 (all other exponentials underflowed, or C = 1); a NaN om stays NaN
__device__ __forceinline__ float focal_pow(float om, float gamma) { return om == 0.f ? 0.f : expf(gamma * logf(om)); }
// log p = log(1 - om): where p is near 1, z - m - log(sum) has already rounded to 0
__device__ __forceinline__ float focal_logp(float om, float logp) { return om < 0.5f ? log1pf(-om) : logp; }

__global__ void zero_f64_kernel(double* p, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) p[i] = 0.0;
}

// per (b,c): {n, sum t logp, sum p t, sum p, sum t} over pixels with t != -1; FOCAL: sum t (1-p)^gamma logp in slot 1
// OHEM (online hard example mining, ohem.h): slots 0 and 1 -- the CE's -- run over the pixels the selection kept, read from
// the stored scores q[B*hw] and the record; the Dice slots 2..4 still run over every valid pixel.  The three arguments behind
// gamma are read by the OHEM instances only.
// PW (per-pixel weights, hrseg.h "border weights"; without OHEM only): slots 0 and 1 become sum pw and sum pw t (1-p)^gamma logp,
// with pw[B*hw] read by the PW instances only.  The weight multiplies t, so the term keeps the shape -- and the roundings --
// of the instance without weights: a map of ones, or of any power of two, gives that instance's bits.
template <int CT, bool FOCAL, bool OHEM, bool PW>
__global__ __launch_bounds__(256) void loss_partials_kernel(const float* __restrict__ z, const float* __restrict__ t,
                                                            double* __restrict__ partial, int C, long hw,
                                                            long pix_per_block, float gamma, const float* __restrict__ q,
                                                            const OhemRecord* __restrict__ rec, float thresh,
                                                            const float* __restrict__ pw) {
  static_assert(!(OHEM && PW), "per-pixel weights are not combined with OHEM");
  __shared__ float red[4][CT * 5];
  const int b = blockIdx.y;
  const long lo = (long)blockIdx.x * pix_per_block;
  const long hi = (lo + pix_per_block < hw) ? lo + pix_per_block : hw;
  float acc[CT][5];
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int k = 0; k < 5; ++k) acc[c][k] = 0.f;
  const float* zb = z + (size_t)b * C * hw;
  const float* tb = t + (size_t)b * C * hw;
  float lam_k = 0.f;
  if constexpr (OHEM) lam_k = rec->lam_k;
  for (long pix = lo + threadIdx.x; pix < hi; pix += 256) {
    bool kept = true;
    if constexpr (OHEM) kept = ohem_kept(q[(size_t)b * hw + pix], thresh, lam_k);
    float wpix = 1.f;
    if constexpr (PW) wpix = pw[(size_t)b * hw + pix];
    float zz[CT], tt[CT];
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      zz[c] = (c < C) ? zb[(size_t)c * hw + pix] : -INFINITY;
      tt[c] = (c < C) ? tb[(size_t)c * hw + pix] : -1.f;
      m = fmaxf(m, zz[c]);
    }
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      zz[c] = zz[c] - m;
      s += (c < C) ? expf(zz[c]) : 0.f;
    }
    const float ls = logf(s), inv = 1.f / s;
    float e[CT], rest[CT], pre = 0.f;
    if constexpr (FOCAL) {
#pragma unroll
      for (int c = 0; c < CT; ++c) e[c] = (c < C) ? expf(zz[c]) : 0.f;
      focal_suffix<CT>(e, rest);
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      if (c < C && tt[c] != -1.f) {
        const float logp = zz[c] - ls, p = expf(zz[c]) * inv;
        if (!OHEM || kept) {
          const float wt = PW ? wpix * tt[c] : tt[c];
          acc[c][0] += PW ? wpix : 1.f;
          if constexpr (FOCAL) {
            if (tt[c] != 0.f) {
              const float om = (pre + rest[c]) * inv;
              acc[c][1] += wt * focal_pow(om, gamma) * focal_logp(om, logp);
            } else {
              acc[c][1] += wt * logp;         // 0, or the NaN of a poisoned pixel
            }
          } else {
            acc[c][1] += wt * logp;
          }
        }
        acc[c][2] += p * tt[c];
        acc[c][3] += p;
        acc[c][4] += tt[c];
      }
      if constexpr (FOCAL) pre += e[c];
    }
  }
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const float v = wave_sum(acc[c][k]);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][c * 5 + k] = v;
    }
  __syncthreads();
  if (threadIdx.x < C * 5) {
    const double v = (double)red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    atomicAdd(partial + (size_t)b * C * 5 + threadIdx.x, v);
  }
}

// out[0]=CE out[1]=Dice out[2]=#valid dice items ; coef[b][c] = {ce, dice_a, dice_b, 0}
// Dice item = 1 - N/D with N = 2I + smooth, D = 2(1-alpha-beta) I + 2 alpha P + 2 beta T + smooth (Tversky weights on the false
// positives P - I and the false negatives T - I); an item counts iff D != 0.  d(item)/dp at a pixel of class c is
// w_c (t (-2/D + 2N(1-alpha-beta)/D^2) + 2 alpha N / D^2): the two coefficient slots the backward multiplies t and 1 with.
// smooth = 0, alpha = beta = 0.5 (`plain`) is 1 - 2I/U with U = P + T, evaluated by the expressions it always was.
__global__ void loss_finalize_kernel(const double* __restrict__ partial, const float* __restrict__ w, int B, int C,
                                     float smooth, float alpha, float beta, float* __restrict__ out,
                                     float* __restrict__ coef) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const bool plain = (smooth == 0.f && alpha == 0.5f && beta == 0.5f);
  const double sm = smooth, al = alpha, be = beta, mix = 1.0 - al - be;
  double ce = 0.0, dice = 0.0;
  int nvalid = 0;
  for (int b = 0; b < B; ++b) {
    double I = 0.0, P = 0.0, T = 0.0, U = 0.0;
    for (int c = 0; c < C; ++c) {
      const double* q = partial + (b * C + c) * 5;
      U += (double)w[c] * (q[3] + q[4]);
      I += (double)w[c] * q[2];
      P += (double)w[c] * q[3];
      T += (double)w[c] * q[4];
    }
    const double D = plain ? U : 2.0 * mix * I + 2.0 * al * P + 2.0 * be * T + sm;
    if (D != 0.0) ++nvalid;
  }
  for (int b = 0; b < B; ++b) {
    bool ok = true;
    double item = 0.0, I = 0.0, U = 0.0, P = 0.0, T = 0.0;
    for (int c = 0; c < C; ++c) {
      const double* q = partial + (b * C + c) * 5;
      if (q[0] <= 0.0) ok = false;
      else item += -(double)w[c] * q[1] / q[0];
      I += (double)w[c] * q[2];
      U += (double)w[c] * (q[3] + q[4]);
      P += (double)w[c] * q[3];
      T += (double)w[c] * q[4];
    }
    ce += ok ? item / C : 1.0;
    const double N = 2.0 * I + sm;
    const double D = plain ? U : 2.0 * mix * I + 2.0 * al * P + 2.0 * be * T + sm;
    const bool dv = (D != 0.0);
    if (dv) dice += plain ? 1.0 - 2.0 * I / U : 1.0 - N / D;
    for (int c = 0; c < C; ++c) {
      const double* q = partial + (b * C + c) * 5;
      float* k = coef + (b * C + c) * 4;
      k[0] = ok ? (float)(-(double)w[c] / (q[0] * C * B)) : 0.f;
      if (plain) {
        k[1] = dv ? (float)(-2.0 * w[c] / (U * nvalid)) : 0.f;
        k[2] = dv ? (float)(2.0 * I * w[c] / (U * U * nvalid)) : 0.f;
      } else {
        k[1] = dv ? (float)((double)w[c] * (-2.0 / D + 2.0 * N * mix / (D * D)) / nvalid) : 0.f;
        k[2] = dv ? (float)((double)w[c] * 2.0 * al * N / (D * D * nvalid)) : 0.f;
      }
      k[3] = 0.f;
    }
  }
  out[0] = (float)(ce / B);
  out[1] = nvalid ? (float)(dice / nvalid) : 0.f;
  out[2] = (float)nvalid;
}

// FOCAL: d(-t (1-p)^gamma log p) / d log p = -t [(1-p)^gamma - gamma p (1-p)^(gamma-1) log p] replaces the CE's -t; the
// softmax Jacobian behind it is the same.  The bracket is (1-p)^gamma (1 - gamma p log p / (1-p)), 0 in the limit 1-p -> 0.
// OHEM: the selection is a constant, so the CE part of dz is simply 0 at the pixels it did not keep (the same stored scores
// and record as the forward: the two cannot disagree); the Dice part is untouched.
// PW: the CE part of dz at a pixel is multiplied by pw there, through the CE's seed g[0] (one register, none more live: through t
// the CT = 16 focal instance went to 168 bytes of scratch); the Dice part is untouched.
template <int CT, bool FOCAL, bool OHEM, bool PW>
__global__ __launch_bounds__(256) void loss_bwd_kernel(const float* __restrict__ z, const float* __restrict__ t,
                                                       const float* __restrict__ coef, const float* __restrict__ g,
                                                       float* __restrict__ dz, int acc, int C, long hw, float gamma,
                                                       const float* __restrict__ q, const OhemRecord* __restrict__ rec,
                                                       float thresh, const float* __restrict__ pw) {
  static_assert(!(OHEM && PW), "per-pixel weights are not combined with OHEM");
  const int b = blockIdx.y;
  const long pix = (long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= hw) return;
  float gce = g[0];
  const float gdice = g[1];
  bool kept = true;
  if constexpr (OHEM) kept = ohem_kept(q[(size_t)b * hw + pix], thresh, rec->lam_k);
  if constexpr (PW) gce *= pw[(size_t)b * hw + pix];
  const float* zb = z + (size_t)b * C * hw + pix;
  const float* tb = t + (size_t)b * C * hw + pix;
  float zz[CT], tt[CT], p[CT];
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    zz[c] = (c < C) ? zb[(size_t)c * hw] : -INFINITY;
    tt[c] = (c < C) ? tb[(size_t)c * hw] : -1.f;
    m = fmaxf(m, zz[c]);
  }
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    p[c] = (c < C) ? expf(zz[c] - m) : 0.f;
    s += p[c];
  }
  const float inv = 1.f / s;
  float dlogp[CT], dpr[CT], sum_dlogp = 0.f, dot = 0.f;
  float rest[CT], pre = 0.f, ls = 0.f;
  if constexpr (FOCAL) {
    focal_suffix<CT>(p, rest);          // p still holds the exponentials
    ls = logf(s);
  }
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const float e = p[c];
    p[c] *= inv;
    dlogp[c] = 0.f;
    dpr[c] = 0.f;
    if (c < C && tt[c] != -1.f) {
      const float* k = coef + ((size_t)b * C + c) * 4;
      dlogp[c] = gce * k[0] * tt[c];
      if constexpr (FOCAL) {
        if (tt[c] != 0.f) {
          const float om = (pre + rest[c]) * inv;
          const float logp = focal_logp(om, zz[c] - m - ls);
          dlogp[c] *= (om == 0.f) ? 0.f : focal_pow(om, gamma) * (1.f - gamma * p[c] * logp / om);
        }
      }
      // (a select behind the arithmetic, not a branch around it: the branch cost the CT = 16 focal instance 408 bytes of scratch)
      if (OHEM && !kept) dlogp[c] = 0.f;
      dpr[c] = gdice * (k[1] * tt[c] + k[2]);
    }
    if constexpr (FOCAL) pre += e;
    sum_dlogp += dlogp[c];
    dot += p[c] * dpr[c];
  }
  float* db = dz + (size_t)b * C * hw + pix;
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if (c < C) {
      const float v = dlogp[c] - p[c] * sum_dlogp + p[c] * (dpr[c] - dot);
      db[(size_t)c * hw] = acc ? db[(size_t)c * hw] + v : v;
    }
}

// The entry points without options are the _opt ones at gamma = 0, smooth = 0, alpha = beta = 0.5; `name` is the one that was
// called (a refusal names it).  An option must be finite and >= 0.
static bool loss_option_ok(float v) { return v >= 0.f && v <= FLT_MAX; }

// The _ohem entry points are the _opt ones with the stored scores, the selection's record and the threshold (`ohem` set): the
// masked instances of the same kernels.
struct OhemArgs { const float* q; const OhemRecord* rec; float thresh; };
static const OhemArgs* const NO_OHEM = nullptr;
// The _pw entry points are the _opt ones with one weight per pixel on the CE term (`pw` set; hrseg.h "border weights"): the PW
// instances of the same kernels.  Never together with `ohem`.
struct PixelWeights { const float* pw; };
static const PixelWeights* const NO_PW = nullptr;

static int loss_partials(const char* name, const float* z, const float* t, double* partial, int B, int C, long hw,
                         float gamma, const OhemArgs* ohem, const PixelWeights* pixw, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(z && t && partial && B > 0 && C > 0 && C <= MAXC && hw > 0, "%s: bad arguments (C=%d)", name, C);
  HRSEG_CHECK_ARG(loss_option_ok(gamma), "%s: gamma must be finite and >= 0 (got %g)", name, (double)gamma);
  if (pixw) HRSEG_CHECK_ARG(pixw->pw && !ohem, "%s: null pointer (pw)", name);
  if (ohem) {
    HRSEG_CHECK_ARG(ohem->q && ohem->rec, "%s: null pointer (q, record)", name);
    HRSEG_CHECK_ARG(ohem_thresh_ok(ohem->thresh), "%s: thresh must be a finite number in [0, 1] (got %g)", name, (double)ohem->thresh);
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(zero_f64_kernel, dim3(1), dim3(256), 0, st, partial, B * C * 5);   // kernel node, not memset
  long chunks = hrseg_g_deterministic ? 1 : 1024 / B;      // deterministic: one block (one adder) per image
  if (chunks < 1) chunks = 1;
  long ppb = (hw + chunks - 1) / chunks;
  if (ppb < 256) ppb = 256;
  dim3 grid(ceil_div(hw, ppb), B);
  const float* q = ohem ? ohem->q : nullptr;
  const OhemRecord* rec = ohem ? ohem->rec : nullptr;
  const float thresh = ohem ? ohem->thresh : 0.f;
  const float* pw = pixw ? pixw->pw : nullptr;
  if (ohem) {
    if (gamma > 0.f) LAUNCH_CT_FLAGS(loss_partials_kernel, true, true, false, C, grid, st, z, t, partial, C, hw, ppb, gamma, q, rec, thresh, pw);
    else LAUNCH_CT_FLAGS(loss_partials_kernel, false, true, false, C, grid, st, z, t, partial, C, hw, ppb, gamma, q, rec, thresh, pw);
    hrseg_count(CNT_OHEM);
  } else if (pixw) {
    if (gamma > 0.f) LAUNCH_CT_FLAGS(loss_partials_kernel, true, false, true, C, grid, st, z, t, partial, C, hw, ppb, gamma, q, rec, thresh, pw);
    else LAUNCH_CT_FLAGS(loss_partials_kernel, false, false, true, C, grid, st, z, t, partial, C, hw, ppb, gamma, q, rec, thresh, pw);
  } else {
    if (gamma > 0.f) LAUNCH_CT_FLAGS(loss_partials_kernel, true, false, false, C, grid, st, z, t, partial, C, hw, ppb, gamma, q, rec, thresh, pw);
    else LAUNCH_CT_FLAGS(loss_partials_kernel, false, false, false, C, grid, st, z, t, partial, C, hw, ppb, gamma, q, rec, thresh, pw);
  }
  HRSEG_LAUNCH_CHECK("loss_partials");
  return 0;
}

static int loss_finalize(const char* name, const double* partial, const float* w, int B, int C, float smooth, float alpha,
                         float beta, float* out, float* coef, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(partial && w && out && coef && B > 0 && C > 0, "%s: bad arguments", name);
  HRSEG_CHECK_ARG(loss_option_ok(smooth) && loss_option_ok(alpha) && loss_option_ok(beta),
                  "%s: smooth, alpha and beta must be finite and >= 0 (got %g, %g, %g)", name, (double)smooth, (double)alpha,
                  (double)beta);
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partial, w, B, C, smooth, alpha, beta,
                     out, coef);
  HRSEG_LAUNCH_CHECK("loss_finalize");
  return 0;
}

static int loss_bwd(const char* name, const float* z, const float* t, const float* coef, const float* g, float* dz,
                    int accumulate, int B, int C, long hw, float gamma, const OhemArgs* ohem, const PixelWeights* pixw,
                    hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(z && t && coef && g && dz && B > 0 && C > 0 && C <= MAXC && hw > 0, "%s: bad arguments", name);
  HRSEG_CHECK_ARG(loss_option_ok(gamma), "%s: gamma must be finite and >= 0 (got %g)", name, (double)gamma);
  if (pixw) HRSEG_CHECK_ARG(pixw->pw && !ohem, "%s: null pointer (pw)", name);
  if (ohem) {
    HRSEG_CHECK_ARG(ohem->q && ohem->rec, "%s: null pointer (q, record)", name);
    HRSEG_CHECK_ARG(ohem_thresh_ok(ohem->thresh), "%s: thresh must be a finite number in [0, 1] (got %g)", name, (double)ohem->thresh);
  }
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(ceil_div(hw, 256), B);
  const float* q = ohem ? ohem->q : nullptr;
  const OhemRecord* rec = ohem ? ohem->rec : nullptr;
  const float thresh = ohem ? ohem->thresh : 0.f;
  const float* pw = pixw ? pixw->pw : nullptr;
  if (ohem) {
    if (gamma > 0.f) LAUNCH_CT_FLAGS(loss_bwd_kernel, true, true, false, C, grid, st, z, t, coef, g, dz, accumulate, C, hw, gamma, q, rec, thresh, pw);
    else LAUNCH_CT_FLAGS(loss_bwd_kernel, false, true, false, C, grid, st, z, t, coef, g, dz, accumulate, C, hw, gamma, q, rec, thresh, pw);
    hrseg_count(CNT_OHEM);
  } else if (pixw) {
    if (gamma > 0.f) LAUNCH_CT_FLAGS(loss_bwd_kernel, true, false, true, C, grid, st, z, t, coef, g, dz, accumulate, C, hw, gamma, q, rec, thresh, pw);
    else LAUNCH_CT_FLAGS(loss_bwd_kernel, false, false, true, C, grid, st, z, t, coef, g, dz, accumulate, C, hw, gamma, q, rec, thresh, pw);
  } else {
    if (gamma > 0.f) LAUNCH_CT_FLAGS(loss_bwd_kernel, true, false, false, C, grid, st, z, t, coef, g, dz, accumulate, C, hw, gamma, q, rec, thresh, pw);
    else LAUNCH_CT_FLAGS(loss_bwd_kernel, false, false, false, C, grid, st, z, t, coef, g, dz, accumulate, C, hw, gamma, q, rec, thresh, pw);
  }
  HRSEG_LAUNCH_CHECK("loss_bwd");
  return 0;
}

extern "C" int hrseg_loss_partials(const float* z, const float* t, double* partial, int B, int C, long hw,
                                   hrseg_stream_t stream) {
  return loss_partials("hrseg_loss_partials", z, t, partial, B, C, hw, 0.f, NO_OHEM, NO_PW, stream);
}
extern "C" int hrseg_loss_partials_opt(const float* z, const float* t, double* partial, int B, int C, long hw, float gamma,
                                       hrseg_stream_t stream) {
  return loss_partials("hrseg_loss_partials_opt", z, t, partial, B, C, hw, gamma, NO_OHEM, NO_PW, stream);
}
extern "C" int hrseg_loss_finalize(const double* partial, const float* w, int B, int C, float* out, float* coef,
                                   hrseg_stream_t stream) {
  return loss_finalize("hrseg_loss_finalize", partial, w, B, C, 0.f, 0.5f, 0.5f, out, coef, stream);
}
extern "C" int hrseg_loss_finalize_opt(const double* partial, const float* w, int B, int C, float smooth, float alpha,
                                       float beta, float* out, float* coef, hrseg_stream_t stream) {
  return loss_finalize("hrseg_loss_finalize_opt", partial, w, B, C, smooth, alpha, beta, out, coef, stream);
}
extern "C" int hrseg_loss_bwd(const float* z, const float* t, const float* coef, const float* g, float* dz,
                              int accumulate, int B, int C, long hw, hrseg_stream_t stream) {
  return loss_bwd("hrseg_loss_bwd", z, t, coef, g, dz, accumulate, B, C, hw, 0.f, NO_OHEM, NO_PW, stream);
}
extern "C" int hrseg_loss_bwd_opt(const float* z, const float* t, const float* coef, const float* g, float* dz,
                                  int accumulate, int B, int C, long hw, float gamma, hrseg_stream_t stream) {
  return loss_bwd("hrseg_loss_bwd_opt", z, t, coef, g, dz, accumulate, B, C, hw, gamma, NO_OHEM, NO_PW, stream);
}
extern "C" int hrseg_loss_partials_ohem(const float* z, const float* t, const float* q, const void* record, float thresh,
                                        double* partial, int B, int C, long hw, float gamma, hrseg_stream_t stream) {
  const OhemArgs ohem = {q, (const OhemRecord*)record, thresh};
  return loss_partials("hrseg_loss_partials_ohem", z, t, partial, B, C, hw, gamma, &ohem, NO_PW, stream);
}
extern "C" int hrseg_loss_bwd_ohem(const float* z, const float* t, const float* q, const void* record, float thresh,
                                   const float* coef, const float* g, float* dz, int accumulate, int B, int C, long hw,
                                   float gamma, hrseg_stream_t stream) {
  const OhemArgs ohem = {q, (const OhemRecord*)record, thresh};
  return loss_bwd("hrseg_loss_bwd_ohem", z, t, coef, g, dz, accumulate, B, C, hw, gamma, &ohem, NO_PW, stream);
}
extern "C" int hrseg_loss_partials_pw(const float* z, const float* t, const float* pw, double* partial, int B, int C, long hw,
                                      float gamma, hrseg_stream_t stream) {
  const PixelWeights pixw = {pw};
  return loss_partials("hrseg_loss_partials_pw", z, t, partial, B, C, hw, gamma, NO_OHEM, &pixw, stream);
}
extern "C" int hrseg_loss_bwd_pw(const float* z, const float* t, const float* pw, const float* coef, const float* g, float* dz,
                                 int accumulate, int B, int C, long hw, float gamma, hrseg_stream_t stream) {
  const PixelWeights pixw = {pw};
  return loss_bwd("hrseg_loss_bwd_pw", z, t, coef, g, dz, accumulate, B, C, hw, gamma, NO_OHEM, &pixw, stream);
}

// --------------------------------------------------------------------------- predictions / confusion counts
// argmax one-hot (masked by t != -1) and confusion counts cm[target][pred]
template <int CT>
__global__ __launch_bounds__(256) void predict_metrics_kernel(const float* __restrict__ z, const float* __restrict__ t,
                                                              float* __restrict__ onehot,
                                                              unsigned long long* __restrict__ cm, int C, long hw,
                                                              long n, int child, int mask_pred) {
  __shared__ unsigned int hist[(MAXC + 1) * (MAXC + 1)];
  const int K = C + (child ? 1 : 0);
  for (int i = threadIdx.x; i < K * K; i += 256) hist[i] = 0;
  __syncthreads();
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long b = i / hw, pix = i - b * hw;
    const float* zb = z + (size_t)b * C * hw + pix;
    const float* tb = t + (size_t)b * C * hw + pix;
    int am = 0;
    float best = zb[0], zsum = 0.f;
    float tt[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      tt[c] = (c < C) ? tb[(size_t)c * hw] : 0.f;
      if (c < C) {
        const float v = zb[(size_t)c * hw];
        zsum += v;
        if (c > 0 && v > best) { best = v; am = c; }
      }
    }
    // prediction label
    int pred;
    if (mask_pred) {
      bool kept = false;  // the arg-max channel survives unless its own target is -1
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c == am) kept = (tt[c] != -1.f);
      if (onehot) {
#pragma unroll
        for (int c = 0; c < CT; ++c)
          if (c < C) onehot[((size_t)b * C + c) * hw + pix] = (c == am && tt[c] != -1.f) ? 1.f : 0.f;
      }
      pred = child ? (kept ? am + 1 : 0) : (kept ? am : 0);
    } else {
      pred = child ? ((zsum == 0.f) ? 0 : am + 1) : am;
    }
    // target label: arg-max (first) of the target with -1 -> 0 when masking, raw otherwise
    int tl = 0;
    float tbest = -INFINITY, tsum = 0.f;
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C) {
        const float v = (mask_pred && tt[c] == -1.f) ? 0.f : tt[c];
        tsum += v;
        if (v > tbest) { tbest = v; tl = c; }
      }
    if (child) {
      // background channel (sum == 0) is prepended: it wins the arg-max when it is 1 (ties -> first)
      const float bg = (tsum == 0.f) ? 1.f : 0.f;
      tl = (bg >= tbest) ? 0 : tl + 1;
    }
    atomicAdd(&hist[tl * K + pred], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K * K; i += 256)
    if (hist[i]) atomicAdd(cm + i, (unsigned long long)hist[i]);
}

extern "C" int hrseg_predict_metrics(const float* z, const float* t, float* onehot, long long* cm, int B, int C,
                                     long hw, int child, int mask_pred, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(z && t && cm && B > 0 && C > 0 && C <= MAXC && hw > 0, "hrseg_predict_metrics: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const long n = (long)B * hw;
  dim3 grid(pixel_blocks(n, 1024));
  unsigned long long* c = (unsigned long long*)cm;
  LAUNCH_CT(predict_metrics_kernel, C, grid, st, z, t, onehot, c, C, hw, n, child, mask_pred);
  HRSEG_LAUNCH_CHECK("predict_metrics");
  return 0;
}

// --------------------------------------------------------------------------- metric vectors
// per-class metric vectors of up to 8 levels from their confusion counts, one launch (Metrics/performance_metrics.py
// metrics_from_confusion: the reference's IoU / Dice / precision / recall classes, train.py:47-51, evaluated in fp64 on the
// counts and rounded to fp32; a zero denominator gives 0).  Thread = one (level, class).
#define METRIC_MAXL 8
struct MetricLevels { int n, total; const long long* cm[METRIC_MAXL]; int K[METRIC_MAXL], child[METRIC_MAXL], off[METRIC_MAXL]; };
__global__ void metric_vectors_kernel(MetricLevels a, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.total) return;
  int L = 0;
  while (L + 1 < a.n && i >= a.off[L + 1]) ++L;
  const int K = a.K[L], ch = a.child[L], c = i - a.off[L] + ch;        // c: label of this class in the K x K matrix
  const long long* cm = a.cm[L];
  // child levels: pixels whose TARGET is the synthetic background label 0 are dropped (rows 1..K-1 only)
  double tp = (double)cm[(long)c * K + c], row = 0.0, col = 0.0;
  for (int j = 0; j < K; ++j) row += (double)cm[(long)c * K + j];
  for (int r = ch; r < K; ++r) col += (double)cm[(long)r * K + c];
  const double fn = row - tp, fp = col - tp;
  auto sdiv = [](double x, double y) { return y == 0.0 ? 0.f : (float)(x / y); };
  const float rec = sdiv(tp, tp + fn);
  out[0 * a.total + i] = rec;                                  // "accuracy" (per-class accuracy = recall, as in the reference)
  out[1 * a.total + i] = sdiv(tp, tp + fp + fn);               // iou
  out[2 * a.total + i] = sdiv(2.0 * tp, 2.0 * tp + fp + fn);   // dice
  out[3 * a.total + i] = sdiv(tp, tp + fp);                    // precision
  out[4 * a.total + i] = rec;                                  // recall
}
extern "C" int hrseg_metric_vectors(int nlevels, const long long* const* cm, const int* K, const int* child, float* out,
                                    hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(nlevels >= 1 && nlevels <= METRIC_MAXL && cm && K && child && out, "hrseg_metric_vectors: 1..%d levels", METRIC_MAXL);
  MetricLevels a;
  a.n = nlevels;
  a.total = 0;
  for (int L = 0; L < nlevels; ++L) {
    HRSEG_CHECK_ARG(cm[L] && K[L] > (child[L] ? 1 : 0) && K[L] <= MAXC + 1, "hrseg_metric_vectors: level %d: bad matrix", L);
    a.cm[L] = cm[L];
    a.K[L] = K[L];
    a.child[L] = child[L] ? 1 : 0;
    a.off[L] = a.total;
    a.total += K[L] - a.child[L];
  }
  hipLaunchKernelGGL(metric_vectors_kernel, dim3((a.total + 63) / 64), dim3(64), 0, (hipStream_t)stream, a, out);
  HRSEG_LAUNCH_CHECK("metric_vectors");
  return 0;
}
