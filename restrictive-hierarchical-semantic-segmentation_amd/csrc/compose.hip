// Everything that walks the class tree's group table: the probability composition over the tree (sigmoid at the roots,
// gated group softmax below), the consistency term and the opt-in grouped KL.  gfx950.
// Each family's kernels are followed by its entry points.
//
// Logits / probabilities here are NCHW fp32 planes ([B,C,hw]) as the reference returns them; C per level is small
// (<= 16), so a thread owns one pixel and walks the C planes (each plane access is coalesced across lanes).
#include "common.h"
#include "level_common.h"
#include "group_table.h"      // struct Groups, fill_groups (shared with distill.hip)

// The prelude the six entry points with a group table share, after the null checks of their own pointers: the sizes
// ("bad arguments"), then the table itself (fill_groups), refused under the entry point's name `who` (a literal).  It reads
// the parameters by the names all six give them and declares the table G and the pixel count n.
#define GROUP_TABLE(who, G)                                                                           \
  HRSEG_CHECK_ARG(B > 0 && C > 0 && C <= MAXC && Cprev > 0 && Cprev <= MAXC && hw > 0 && ngroups > 0, \
                  who ": bad arguments");                                                             \
  Groups G;                                                                                           \
  if (int e = fill_groups(G, ngroups, group_parent, group_size, C, Cprev, who)) return e;             \
  const long n = (long)B * hw

// --------------------------------------------------------------------------- composition
__global__ void sigmoid_fwd_kernel(const float* __restrict__ z, float* __restrict__ p, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 1.f / (1.f + expf(-z[i]));
}
// dz (=|+=) dp * p (1-p); dp element (b,c,i) at b*sb + c*sc + i*si
__global__ void sigmoid_bwd_kernel(const float* __restrict__ dp, long sb, long sc, long si,
                                   const float* __restrict__ z, float* __restrict__ dz, int acc, int C, long hw,
                                   long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long bc = i / hw, pix = i - bc * hw;
  const long b = bc / C, c = bc - b * C;
  const float p = 1.f / (1.f + expf(-z[i]));
  const float g = dp[b * sb + c * sc + pix * si] * p * (1.f - p);
  dz[i] = acc ? dz[i] + g : g;
}

extern "C" int hrseg_sigmoid_fwd(const float* z, float* p, long n, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(z && p && n > 0, "hrseg_sigmoid_fwd: bad arguments");
  hipLaunchKernelGGL(sigmoid_fwd_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, z, p, n);
  HRSEG_LAUNCH_CHECK("sigmoid_fwd");
  return 0;
}

extern "C" int hrseg_sigmoid_bwd(const float* dp, long sb, long sc, long si, const float* z, float* dz, int accumulate,
                                 int B, int C, long hw, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(dp && z && dz && B > 0 && C > 0 && hw > 0, "hrseg_sigmoid_bwd: bad arguments");
  const long n = (long)B * C * hw;
  hipLaunchKernelGGL(sigmoid_bwd_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, dp, sb, sc, si, z,
                     dz, accumulate, C, hw, n);
  HRSEG_LAUNCH_CHECK("sigmoid_bwd");
  return 0;
}

#define EPS_GATE 1e-6f
__global__ void compose_fwd_kernel(const float* __restrict__ z, const float* __restrict__ pprev,
                                   float* __restrict__ p, int C, int Cprev, long hw, long n, Groups g) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long b = i / hw, pix = i - b * hw;
  const float* zb = z + (size_t)b * C * hw + pix;
  float* pb = p + (size_t)b * C * hw + pix;
  int start = 0;
  for (int gi = 0; gi < g.n; ++gi) {
    const int sz = g.size[gi];
    const float pp = pprev[((size_t)b * Cprev + g.parent[gi]) * hw + pix];
    const float lg = logf(pp + EPS_GATE);
    float m = -INFINITY;
    for (int c = 0; c < sz; ++c) m = fmaxf(m, zb[(size_t)(start + c) * hw] + lg);
    float s = 0.f;
    for (int c = 0; c < sz; ++c) s += expf(zb[(size_t)(start + c) * hw] + lg - m);
    const float inv = 1.f / s;
    for (int c = 0; c < sz; ++c) pb[(size_t)(start + c) * hw] = pp * (expf(zb[(size_t)(start + c) * hw] + lg - m) * inv);
    start += sz;
  }
}
__global__ void compose_bwd_kernel(const float* __restrict__ dp, long sb, long sc, long si,
                                   const float* __restrict__ z, const float* __restrict__ pprev,
                                   float* __restrict__ dz, int dz_acc, float* __restrict__ dpprev, int dpp_acc,
                                   int C, int Cprev, long hw, long n, Groups g) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long b = i / hw, pix = i - b * hw;
  const float* zb = z + (size_t)b * C * hw + pix;
  float dpar[MAXC];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) dpar[c] = 0.f;
  int start = 0;
  for (int gi = 0; gi < g.n; ++gi) {
    const int sz = g.size[gi];
    const float pp = pprev[((size_t)b * Cprev + g.parent[gi]) * hw + pix];
    const float lg = logf(pp + EPS_GATE);
    float m = -INFINITY;
    for (int c = 0; c < sz; ++c) m = fmaxf(m, zb[(size_t)(start + c) * hw] + lg);
    float s = 0.f;
    for (int c = 0; c < sz; ++c) s += expf(zb[(size_t)(start + c) * hw] + lg - m);
    const float inv = 1.f / s;
    // dq_c = dP_c * pp ; ds_c = q_c (dq_c - sum_j q_j dq_j)
    float dot = 0.f, dpp = 0.f;
    for (int c = 0; c < sz; ++c) {
      const float q = expf(zb[(size_t)(start + c) * hw] + lg - m) * inv;
      const float d = dp[b * sb + (start + c) * sc + pix * si];
      dot += q * d * pp;
      dpp += d * q;
    }
    float sum_ds = 0.f;
    for (int c = 0; c < sz; ++c) {
      const float q = expf(zb[(size_t)(start + c) * hw] + lg - m) * inv;
      const float d = dp[b * sb + (start + c) * sc + pix * si];
      const float ds = q * (d * pp - dot);
      sum_ds += ds;
      if (dz) {
        float* o = dz + ((size_t)b * C + start + c) * hw + pix;
        *o = dz_acc ? *o + ds : ds;
      }
    }
    dpp += sum_ds / (pp + EPS_GATE);
    // several groups never share a parent, but keep += for safety
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c == g.parent[gi]) dpar[c] += dpp;
    start += sz;
  }
  if (dpprev) {
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c < Cprev) {
        float* o = dpprev + ((size_t)b * Cprev + c) * hw + pix;
        *o = dpp_acc ? *o + dpar[c] : dpar[c];
      }
  }
}

extern "C" int hrseg_compose_fwd(const float* z, const float* pprev, float* p, int B, int C, int Cprev, long hw,
                                 int ngroups, const int* group_parent, const int* group_size, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(z && pprev && p, "hrseg_compose_fwd: bad arguments");
  GROUP_TABLE("hrseg_compose_fwd", g);
  hipLaunchKernelGGL(compose_fwd_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, z, pprev, p, C,
                     Cprev, hw, n, g);
  HRSEG_LAUNCH_CHECK("compose_fwd");
  return 0;
}

extern "C" int hrseg_compose_bwd(const float* dp, long sb, long sc, long si, const float* z, const float* pprev,
                                 float* dz, int dz_accumulate, float* dpprev, int dpprev_accumulate, int B, int C,
                                 int Cprev, long hw, int ngroups, const int* group_parent, const int* group_size,
                                 hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(dp && z && pprev, "hrseg_compose_bwd: bad arguments");
  GROUP_TABLE("hrseg_compose_bwd", g);
  hipLaunchKernelGGL(compose_bwd_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, dp, sb, sc, si, z,
                     pprev, dz, dz_accumulate, dpprev, dpprev_accumulate, C, Cprev, hw, n, g);
  HRSEG_LAUNCH_CHECK("compose_bwd");
  return 0;
}

// --------------------------------------------------------------------------- consistency term
// sum over pixels of | sum_{c in group} P[b,c] - Pprev[b,parent] | per group
__global__ __launch_bounds__(256) void consistency_kernel(const float* __restrict__ p, const float* __restrict__ pprev,
                                                          double* __restrict__ out, int C, int Cprev, long hw, long n,
                                                          Groups g) {
  __shared__ float red[4][MAXC];
  float acc[MAXC];
#pragma unroll
  for (int k = 0; k < MAXC; ++k) acc[k] = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long b = i / hw, pix = i - b * hw;
    int start = 0;
#pragma unroll
    for (int gi = 0; gi < MAXC; ++gi)
      if (gi < g.n) {
        float s = 0.f;
        for (int c = 0; c < g.size[gi]; ++c) s += p[((size_t)b * C + start + c) * hw + pix];
        acc[gi] += fabsf(s - pprev[((size_t)b * Cprev + g.parent[gi]) * hw + pix]);
        start += g.size[gi];
      }
  }
#pragma unroll
  for (int gi = 0; gi < MAXC; ++gi) {
    const float v = wave_sum(acc[gi]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][gi] = v;
  }
  __syncthreads();
  if (threadIdx.x < g.n)
    atomicAdd(out + threadIdx.x,
              (double)red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// gradient of sum_g (scale_g) * sum_pix |sum_{c in g} P[c] - Pprev[parent_g]|:
// dP[c] = g*scale*sign(diff), dPprev[parent] -= g*scale*sign(diff); upstream scalar g on the device
__global__ void consistency_bwd_kernel(const float* __restrict__ p, const float* __restrict__ pprev,
                                       const float* __restrict__ gup, float scale, float* __restrict__ dp,
                                       float* __restrict__ dpprev, int C, int Cprev, long hw, long n, Groups g) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long b = i / hw, pix = i - b * hw;
  const float gs = gup[0] * scale;
  float dpar[MAXC];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) dpar[c] = 0.f;
  int start = 0;
  for (int gi = 0; gi < g.n; ++gi) {
    float s = 0.f;
    for (int c = 0; c < g.size[gi]; ++c) s += p[((size_t)b * C + start + c) * hw + pix];
    const float d = s - pprev[((size_t)b * Cprev + g.parent[gi]) * hw + pix];
    const float sg = (d > 0.f) ? gs : (d < 0.f ? -gs : 0.f);
    for (int c = 0; c < g.size[gi]; ++c) dp[((size_t)b * C + start + c) * hw + pix] = sg;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c == g.parent[gi]) dpar[c] -= sg;
    start += g.size[gi];
  }
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
    if (c < Cprev) dpprev[((size_t)b * Cprev + c) * hw + pix] = dpar[c];
}

extern "C" int hrseg_consistency(const float* p, const float* pprev, double* out, int B, int C, int Cprev, long hw,
                                 int ngroups, const int* group_parent, const int* group_size, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(p && pprev && out, "hrseg_consistency: bad arguments");
  GROUP_TABLE("hrseg_consistency", g);
  int blocks = pixel_blocks(n, 1024);
  if (hrseg_g_deterministic) blocks = 1;
  hipLaunchKernelGGL(consistency_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, pprev, out, C, Cprev,
                     hw, n, g);
  HRSEG_LAUNCH_CHECK("consistency");
  return 0;
}

extern "C" int hrseg_consistency_bwd(const float* p, const float* pprev, const float* g, float scale, float* dp,
                                     float* dpprev, int B, int C, int Cprev, long hw, int ngroups,
                                     const int* group_parent, const int* group_size, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(p && pprev && g && dp && dpprev, "hrseg_consistency_bwd: bad arguments");
  GROUP_TABLE("hrseg_consistency_bwd", gr);
  hipLaunchKernelGGL(consistency_bwd_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, p, pprev, g,
                     scale, dp, dpprev, C, Cprev, hw, n, gr);
  HRSEG_LAUNCH_CHECK("consistency_bwd");
  return 0;
}

// --------------------------------------------------------------------------- grouped conditional KL (opt-in stabiliser)
// Restates the commented-out `grouped_conditional_kl` of the reference (Metrics/losses.py:180-210): per parent group g
// of the level, Q = softmax_c(z_c + log(P_parent + 1e-6)).clamp_min(1e-8) over the group's children and
// KL(Q || Uniform) = Q * (log Q - log(1/g)), `.mean()` over [B, g, H, W]; the level's value is the mean over its groups.
// (The log-bias is the same for every child of a group, so Q = softmax(z) and P_parent receives no gradient.)
// out[gi] += sum over pixels and children of Qc * (log Qc + log g), double.
__global__ __launch_bounds__(256) void group_kl_kernel(const float* __restrict__ z, const float* __restrict__ pprev,
                                                       double* __restrict__ out, int C, int Cprev, long hw, long n, Groups g) {
  __shared__ float red[4][MAXC];
  float acc[MAXC];
#pragma unroll
  for (int k = 0; k < MAXC; ++k) acc[k] = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long b = i / hw, pix = i - b * hw;
    int start = 0;
#pragma unroll
    for (int gi = 0; gi < MAXC; ++gi)
      if (gi < g.n) {
        const int gs = g.size[gi];
        const float lb = logf(pprev[((size_t)b * Cprev + g.parent[gi]) * hw + pix] + 1e-6f);
        float v[MAXC], m = -INFINITY;
        for (int c = 0; c < gs; ++c) {
          v[c] = z[((size_t)b * C + start + c) * hw + pix] + lb;
          m = fmaxf(m, v[c]);
        }
        float den = 0.f;
        for (int c = 0; c < gs; ++c) { v[c] = expf(v[c] - m); den += v[c]; }
        const float lg = logf((float)gs);
        float kl = 0.f;
        for (int c = 0; c < gs; ++c) {
          const float qq = v[c] / den;
          const float q = qq < 1e-8f ? 1e-8f : qq;       // clamp_min that keeps NaN, as torch's (fmaxf would answer 1e-8)
          kl += q * (logf(q) + lg);
        }
        acc[gi] += kl;
        start += gs;
      }
  }
#pragma unroll
  for (int gi = 0; gi < MAXC; ++gi) {
    const float v = wave_sum(acc[gi]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][gi] = v;
  }
  __syncthreads();
  if (threadIdx.x < g.n)
    atomicAdd(out + threadIdx.x,
              (double)red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// dz of  gup * sum_g scale_g * sum_{pix,c} Qc (log Qc + log g),  scale_g = scale / (size_g)  (the .mean() over the
// channel dimension; `scale` carries 1 / (B*H*W*ngroups)).  With a_c = [Q_c >= 1e-8] (log Qc_c + 1 + log g):
// dz_j = Q_j (a_j - sum_c a_c Q_c).
__global__ void group_kl_bwd_kernel(const float* __restrict__ z, const float* __restrict__ pprev,
                                    const float* __restrict__ gup, float scale, float* __restrict__ dz, int C, int Cprev,
                                    long hw, long n, Groups g) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long b = i / hw, pix = i - b * hw;
  const float gsc = gup[0] * scale;
  int start = 0;
  for (int gi = 0; gi < g.n; ++gi) {
    const int gs = g.size[gi];
    const float lb = logf(pprev[((size_t)b * Cprev + g.parent[gi]) * hw + pix] + 1e-6f);
    float v[MAXC], m = -INFINITY;
    for (int c = 0; c < gs; ++c) {
      v[c] = z[((size_t)b * C + start + c) * hw + pix] + lb;
      m = fmaxf(m, v[c]);
    }
    float den = 0.f;
    for (int c = 0; c < gs; ++c) { v[c] = expf(v[c] - m); den += v[c]; }
    const float lg = logf((float)gs);
    float a[MAXC], dot = 0.f;
    for (int c = 0; c < gs; ++c) {
      const float q = v[c] / den;
      v[c] = q;
      a[c] = (q >= 1e-8f) ? (logf(q) + 1.f + lg) : 0.f;
      dot += a[c] * q;
    }
    const float sc = gsc / (float)gs;
    for (int c = 0; c < gs; ++c) dz[((size_t)b * C + start + c) * hw + pix] = sc * v[c] * (a[c] - dot);
    start += gs;
  }
}

extern "C" int hrseg_group_kl(const float* z, const float* pprev, double* out, int B, int C, int Cprev, long hw,
                              int ngroups, const int* group_parent, const int* group_size, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(z && pprev && out, "hrseg_group_kl: bad arguments");
  GROUP_TABLE("hrseg_group_kl", g);
  int blocks = pixel_blocks(n, 1024);
  if (hrseg_g_deterministic) blocks = 1;
  hipLaunchKernelGGL(group_kl_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, z, pprev, out, C, Cprev, hw, n, g);
  HRSEG_LAUNCH_CHECK("group_kl");
  return 0;
}

extern "C" int hrseg_group_kl_bwd(const float* z, const float* pprev, const float* g, float scale, float* dz, int B, int C,
                                  int Cprev, long hw, int ngroups, const int* group_parent, const int* group_size,
                                  hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(z && pprev && g && dz, "hrseg_group_kl_bwd: bad arguments");
  GROUP_TABLE("hrseg_group_kl_bwd", gr);
  hipLaunchKernelGGL(group_kl_bwd_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, z, pprev, g, scale, dz,
                     C, Cprev, hw, n, gr);
  HRSEG_LAUNCH_CHECK("group_kl_bwd");
  return 0;
}
