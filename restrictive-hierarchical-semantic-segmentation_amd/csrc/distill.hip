// Tree distillation (hrseg.h, "tree distillation"): per sibling group of one level the KL between the teacher's and the
// student's conditional distribution over the children, weighted by the teacher's composed probability of the parent and
// gated by the teacher's confidence; forward sums and the gradient w.r.t. the student logits.  gfx950.
//
// Logits are NCHW fp32 planes ([B,C,hw]); as in loss.hip a thread owns one pixel and holds both channel sets -- CT = the
// level's channel count rounded up to 4 / 8 / 16 -- in registers.  The groups are runs of consecutive channels, so every
// per-group quantity (maximum, sum of exponentials, KL) is a SEGMENTED scan over the statically unrolled channel loop: bit c
// of `first` / `last` says whether channel c opens / closes its group (the last register, CT-1, closes whatever is open).
// The bits are uniform, every register index is a compile-time constant, and nothing is indexed by a group number: no
// scratch.  The pad channels C..CT-1 form a group of their own that nothing reads.
#include <cfloat>

#include "common.h"
#include "level_common.h"
#include "group_table.h"

// a_c = beta * u_c and a_c - max must stay two roundings: fused, a group of one would give beta*u - fl(beta*u) != 0, and the
// teacher's and the student's chains would no longer be the same function of their inputs (u == z gives exactly 0).
#pragma clang fp contract(off)

struct TreeTable {
  unsigned first, last;   // bit c: channel c opens / closes a group (bits C.. : the pad group)
  int cpar[MAXC];         // parent channel of the group channel c belongs to (0 where no parents are read)
};

// m[c] = max over the group of c
template <int CT>
__device__ __forceinline__ void seg_max(const float (&x)[CT], unsigned first, unsigned last, float (&m)[CT]) {
  float r = -INFINITY;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    r = ((first >> c) & 1u) ? x[c] : fmaxf(r, x[c]);
    m[c] = r;
  }
#pragma unroll
  for (int c = CT - 2; c >= 0; --c)
    if (!((last >> c) & 1u)) m[c] = m[c + 1];
}

// One side's group softmax in the log domain: x_c = beta*v_c - max, e_c = exp(x_c), and per group log(sum e) and 1 / sum e
// (evaluated where a group closes, then handed down to its other channels).  lsm[c] = x_c - log(sum e) where WANT_L,
// prob[c] = e_c * (1 / sum e) where WANT_P; an array that is not wanted is not touched.
template <int CT, bool WANT_L, bool WANT_P>
__device__ __forceinline__ void group_log_softmax(const float (&v)[CT], float beta, unsigned first, unsigned last,
                                                  float (&lsm)[CT], float (&prob)[CT]) {
  float mx[CT], x[CT], e[CT];
  seg_max<CT>(v, first, last, mx);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    x[c] = beta * v[c] - beta * mx[c];      // beta > 0 and rounding is monotone: beta * max_c v_c IS max_c (beta * v_c)
    e[c] = expf(x[c]);
    s = ((first >> c) & 1u) ? e[c] : s + e[c];
    mx[c] = s;                              // (the maximum is spent: the register holds the running sum now)
  }
  float ls = 0.f, inv = 0.f;
#pragma unroll
  for (int c = CT - 1; c >= 0; --c) {
    if (c == CT - 1 || ((last >> c) & 1u)) {
      if constexpr (WANT_L) ls = logf(mx[c]);
      if constexpr (WANT_P) inv = 1.f / mx[c];
    }
    if constexpr (WANT_L) lsm[c] = x[c] - ls;
    if constexpr (WANT_P) prob[c] = e[c] * inv;
  }
}

// sum over the group of exp(u_c - max u_c), valid where a group closes: the gate's denominator, at temperature 1 whatever beta
template <int CT>
__device__ __forceinline__ void gate_sums(const float (&u)[CT], unsigned first, unsigned last, float (&sg)[CT]) {
  float mx[CT];
  seg_max<CT>(u, first, last, mx);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const float e = expf(u[c] - mx[c]);
    s = ((first >> c) & 1u) ? e : s + e;
    sg[c] = s;
  }
}

// out[g][3] += {sum m omega kl, sum m omega, count} over the kept pixels of group g.  Grid (chunks of an image, images);
// under the deterministic knob ONE block walks every image, so each slot has a single adder.
template <int CT, bool GATE>
__global__ __launch_bounds__(256) void tree_kl_kernel(const float* __restrict__ z, const float* __restrict__ u,
                                                      const float* __restrict__ wprev, const float* __restrict__ pw,
                                                      double* __restrict__ out, int B, int C, int Cprev, long hw,
                                                      long pix_per_block, float beta, float thresh, TreeTable G) {
  __shared__ double red[4][CT * 3];
  const unsigned first = G.first, last = G.last;
  double acc0[CT], acc1[CT];
  unsigned cnt[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    acc0[c] = 0.0;
    acc1[c] = 0.0;
    cnt[c] = 0u;
  }
  const long lo = (long)blockIdx.x * pix_per_block;
  const long hi = (lo + pix_per_block < hw) ? lo + pix_per_block : hw;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const float* zb = z + (size_t)b * C * hw;
    const float* ub = u + (size_t)b * C * hw;
    for (long pix = lo + threadIdx.x; pix < hi; pix += 256) {
      const float m = pw ? pw[(size_t)b * hw + pix] : 1.f;
      float zz[CT], uu[CT];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        zz[c] = (c < C) ? zb[(size_t)c * hw + pix] : 0.f;
        uu[c] = (c < C) ? ub[(size_t)c * hw + pix] : 0.f;
      }
      float lq[CT], q[CT], lp[CT], sg[CT];
      group_log_softmax<CT, true, true>(uu, beta, first, last, lq, q);
      group_log_softmax<CT, true, false>(zz, beta, first, last, lp, lp);
      if constexpr (GATE) gate_sums<CT>(uu, first, last, sg);
      float kl = 0.f, om = 1.f;
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        if (c < C) {
          const float t = q[c] * (lq[c] - lp[c]);
          if ((first >> c) & 1u) {
            kl = t;
            om = wprev ? wprev[((size_t)b * Cprev + G.cpar[c]) * hw + pix] : 1.f;
          } else {
            kl += t;
          }
          if ((last >> c) & 1u) {
            bool keep = true;
            if constexpr (GATE) keep = !(om / sg[c] < thresh);
            const float mo = m * om;
            acc0[c] += keep ? (double)(mo * kl) : 0.0;
            acc1[c] += keep ? (double)mo : 0.0;
            cnt[c] += keep ? 1u : 0u;
          }
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if (c < C && ((last >> c) & 1u)) {
      const double v0 = wave_sum_d(acc0[c]), v1 = wave_sum_d(acc1[c]), v2 = wave_sum_d((double)cnt[c]);
      if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][c * 3 + 0] = v0;
        red[threadIdx.x >> 6][c * 3 + 1] = v1;
        red[threadIdx.x >> 6][c * 3 + 2] = v2;
      }
    }
  __syncthreads();
  if (threadIdx.x < CT * 3) {
    const int c = threadIdx.x / 3, k = threadIdx.x - c * 3;
    if (c < C && ((last >> c) & 1u)) {
      const int gi = __popc(first & ((2u << c) - 1u)) - 1;      // groups opened up to channel c, less one
      atomicAdd(out + gi * 3 + k, red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
    }
  }
}

// dz[b,j,i] (=|+=) g[0] * scale * m * omega * beta * (p_j - q_j) on the kept groups; a dropped group writes 0 / adds nothing
template <int CT, bool GATE>
__global__ __launch_bounds__(256) void tree_kl_bwd_kernel(const float* __restrict__ z, const float* __restrict__ u,
                                                          const float* __restrict__ wprev, const float* __restrict__ pw,
                                                          const float* __restrict__ g, float scale, float* __restrict__ dz,
                                                          int acc, int C, int Cprev, long hw, float beta, float thresh,
                                                          TreeTable G) {
  const unsigned first = G.first, last = G.last;
  const int b = blockIdx.y;
  const long pix = (long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= hw) return;
  const float gsc = g[0] * scale;
  const float m = pw ? pw[(size_t)b * hw + pix] : 1.f;
  const float* zb = z + (size_t)b * C * hw + pix;
  const float* ub = u + (size_t)b * C * hw + pix;
  float zz[CT], uu[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    zz[c] = (c < C) ? zb[(size_t)c * hw] : 0.f;
    uu[c] = (c < C) ? ub[(size_t)c * hw] : 0.f;
  }
  float q[CT], p[CT], sg[CT];
  group_log_softmax<CT, false, true>(uu, beta, first, last, q, q);
  group_log_softmax<CT, false, true>(zz, beta, first, last, p, p);
  if constexpr (GATE) gate_sums<CT>(uu, first, last, sg);
  // the group's weight and keep flag: the parent is read where the group opens, the gate decided where it closes, both
  // handed down to the group's other channels
  float w[CT];
  bool keep[CT];
  float om = 1.f;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    if (c < C && ((first >> c) & 1u)) om = wprev ? wprev[((size_t)b * Cprev + G.cpar[c]) * hw + pix] : 1.f;
    w[c] = gsc * (m * om) * beta;
    keep[c] = true;
    if constexpr (GATE)
      if (c == CT - 1 || ((last >> c) & 1u)) keep[c] = !(om / sg[c] < thresh);
  }
#pragma unroll
  for (int c = CT - 2; c >= 0; --c)
    if (!((last >> c) & 1u)) keep[c] = keep[c + 1];
  float* db = dz + (size_t)b * C * hw + pix;
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if (c < C) {
      const float v = w[c] * (p[c] - q[c]);
      if (keep[c]) db[(size_t)c * hw] = acc ? db[(size_t)c * hw] + v : v;
      else if (!acc) db[(size_t)c * hw] = 0.f;
    }
}

// launches KERNEL<CT, GATE> (256-thread blocks, no dynamic LDS) with the smallest CT of 4 / 8 / 16 that holds C channels
#define LAUNCH_CT_GATE(KERNEL, GATE, C, grid, st, ...)                                              \
  do {                                                                                              \
    if ((C) <= 4) hipLaunchKernelGGL((KERNEL<4, GATE>), grid, dim3(256), 0, st, __VA_ARGS__);       \
    else if ((C) <= 8) hipLaunchKernelGGL((KERNEL<8, GATE>), grid, dim3(256), 0, st, __VA_ARGS__);  \
    else hipLaunchKernelGGL((KERNEL<16, GATE>), grid, dim3(256), 0, st, __VA_ARGS__);               \
  } while (0)

// What the two entry points refuse alike, each under its own name `who`, and the launch table they share.  Without parents
// (wprev == NULL) the table's parent column is not read and Cprev is ignored.
static int tree_table(const char* who, TreeTable& T, const float* wprev, int B, int C, int Cprev, long hw, int ngroups,
                      const int* group_parent, const int* group_size, float inv_temp, float thresh) {
  HRSEG_CHECK_ARG(B >= 1 && C >= 1 && C <= MAXC && hw >= 1, "%s: bad arguments (B=%d, C=%d, hw=%ld)", who, B, C, hw);
  HRSEG_CHECK_ARG(ngroups >= 1, "%s: bad group table", who);
  if (wprev) HRSEG_CHECK_ARG(Cprev >= 1 && Cprev <= MAXC, "%s: wprev is set and Cprev=%d is outside 1..%d", who, Cprev, MAXC);
  static const int no_parents[MAXC] = {0};
  Groups gr;
  if (int e = fill_groups(gr, ngroups, wprev ? group_parent : no_parents, group_size, C, wprev ? Cprev : 1, who)) return e;
  HRSEG_CHECK_ARG(inv_temp > 0.f && inv_temp <= FLT_MAX, "%s: inv_temp must be finite and > 0 (got %g)", who, (double)inv_temp);
  HRSEG_CHECK_ARG(thresh >= 0.f && thresh <= 1.f, "%s: thresh must be in [0, 1] (got %g)", who, (double)thresh);
  T.first = T.last = 0u;
  int c = 0;
  for (int i = 0; i < gr.n; ++i) {
    T.first |= 1u << c;
    for (int k = 0; k < gr.size[i]; ++k) T.cpar[c++] = gr.parent[i];
    T.last |= 1u << (c - 1);
  }
  if (c < MAXC) T.first |= 1u << c;       // the pad channels: a group of their own
  for (; c < MAXC; ++c) T.cpar[c] = 0;
  return 0;
}

extern "C" int hrseg_tree_kl(const float* z, const float* u, const float* wprev, const float* pw, float inv_temp, float thresh,
                             double* out, int B, int C, int Cprev, long hw, int ngroups, const int* group_parent,
                             const int* group_size, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(z && u && out, "hrseg_tree_kl: null pointer (z, u, out)");
  TreeTable T;
  if (int e = tree_table("hrseg_tree_kl", T, wprev, B, C, Cprev, hw, ngroups, group_parent, group_size, inv_temp, thresh)) return e;
  hipStream_t st = (hipStream_t)stream;
  long chunks = hrseg_g_deterministic ? 1 : 1024 / B;      // deterministic: one block in all (one adder per slot)
  if (chunks < 1) chunks = 1;
  long ppb = (hw + chunks - 1) / chunks;
  if (ppb < 256) ppb = 256;
  dim3 grid(ceil_div(hw, ppb), hrseg_g_deterministic ? 1 : B);
  if (thresh > 0.f) LAUNCH_CT_GATE(tree_kl_kernel, true, C, grid, st, z, u, wprev, pw, out, B, C, Cprev, hw, ppb, inv_temp, thresh, T);
  else LAUNCH_CT_GATE(tree_kl_kernel, false, C, grid, st, z, u, wprev, pw, out, B, C, Cprev, hw, ppb, inv_temp, thresh, T);
  hrseg_count(CNT_TREE_KL);
  HRSEG_LAUNCH_CHECK("hrseg_tree_kl");
  return 0;
}

extern "C" int hrseg_tree_kl_bwd(const float* z, const float* u, const float* wprev, const float* pw, float inv_temp,
                                 float thresh, const float* g, float scale, float* dz, int accumulate, int B, int C, int Cprev,
                                 long hw, int ngroups, const int* group_parent, const int* group_size, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(z && u && g && dz, "hrseg_tree_kl_bwd: null pointer (z, u, g, dz)");
  TreeTable T;
  if (int e = tree_table("hrseg_tree_kl_bwd", T, wprev, B, C, Cprev, hw, ngroups, group_parent, group_size, inv_temp, thresh)) return e;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(ceil_div(hw, 256), B);
  if (thresh > 0.f) LAUNCH_CT_GATE(tree_kl_bwd_kernel, true, C, grid, st, z, u, wprev, pw, g, scale, dz, accumulate, C, Cprev, hw, inv_temp, thresh, T);
  else LAUNCH_CT_GATE(tree_kl_bwd_kernel, false, C, grid, st, z, u, wprev, pw, g, scale, dz, accumulate, C, Cprev, hw, inv_temp, thresh, T);
  hrseg_count(CNT_TREE_KL);
  HRSEG_LAUNCH_CHECK("hrseg_tree_kl_bwd");
  return 0;
}
