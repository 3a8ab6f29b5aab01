// The optimiser on flat fp32 buffers, for gfx950: AdamW (host scalars, or step count and hyper-parameters in device memory),
// global-norm gradient clipping with the non-finite step skip, the weight EMA, and the fill that zeroes its buffers.
// adamw_body is the spelling of the update: an AdamW kernel here is loads of its scalars plus that body, so the variants
// round alike by construction -- except adamw_dev_kernel, which keeps the same text written out (measured reason there).
//
// Clipping: three launches over the flat gradient buffer g[n] that AdamW is about to consume:
//   1. grad_sumsq_kernel       partial[c] = sum over chunk c of (double)g_i * (double)g_i
//   2. grad_clip_finalize_kernel  S = sum of the partials in a fixed order -> clip = {norm, coef, finite, skipped_total},
//                              and the work of adam_tick_kernel (advance state) unless the step is void
//   3. adamw_dev_clip_kernel   adamw_dev_kernel with gg = (g * grad_scale) * coef and an early return for a void step
//
// Chunk c is elements [c * GRAD_CHUNK, min(n, (c + 1) * GRAD_CHUNK)): length and count depend on n alone, never on the
// launch grid, and within a chunk every element has a fixed place in a fixed summation tree (thread t takes the
// 16-byte pieces t, t + 256, ... in order; xor-shuffle tree per wave; the four wave sums are added in wave order).  No
// atomics anywhere: the result is bit-reproducible from run to run and equal on every rank that holds the same bytes,
// whatever the "deterministic" knob says.  Every element is widened to fp64 BEFORE it is squared, so a finite fp32
// gradient can neither overflow nor underflow the sum (|g| <= 3.4e38 -> g^2 <= 1.2e77, n <= 2^63; the smallest
// subnormal squared is 2e-90), and S is finite exactly when every element is.
//
// Weight EMA: the shadow e[n] of the parameters is advanced by the update kernel itself
// (adamw_dev_ema_kernel / adamw_dev_clip_ema_kernel: one more 16-byte load and store per element group, no launch of
// its own), by ema_update_kernel for an already updated p, and exchanged with p by swap_kernel.
#include "elem_common.h"   // ld4 / st4, flat_blocks, al16

#define GRAD_CHUNK 8192          // floats per partial: 256 threads x 8 pieces of 16 bytes
#define GRAD_MAX_BLOCKS 2048     // 256 CUs x 8 resident blocks of 256 threads; more chunks than this: a block takes several

__device__ __forceinline__ double sq4(double acc, f32x4 v) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double d = (double)v[j];
    acc = fma(d, d, acc);
  }
  return acc;
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, long n,
                                                         double* __restrict__ partial, int nchunks) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const long lo = (long)c * GRAD_CHUNK;
    const float* src = g + lo;
    double acc = 0.0;
    if (lo + GRAD_CHUNK <= n) {                   // block-uniform: eight unguarded 16-byte loads in flight per thread
      f32x4 v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = ld4(src + 4 * (t + 256 * k));
      __builtin_amdgcn_sched_barrier(0);          // all eight loads are issued before the first one is waited for
#pragma unroll
      for (int k = 0; k < 8; ++k) acc = sq4(acc, v[k]);
    } else {                                      // the last chunk: whole pieces, then a scalar tail of len % 4 elements
      // 1 .. GRAD_CHUNK - 1, taken here as an int: as a 64-bit min(n - lo, GRAD_CHUNK) ahead of the branch the compiler's
      // scalar select read a stale condition code and this path ran with the full length (caught by the n = 1 test)
      const int len = (int)(n - lo);
      const int nvec = len >> 2;
      for (int i = t; i < nvec; i += 256) acc = sq4(acc, ld4(src + 4 * i));
      const int tail = len & 3;
      if (t < tail) {
        const double d = (double)src[4 * nvec + t];
        acc = fma(d, d, acc);
      }
    }
    acc = wave_sum_d(acc);
    if ((t & 63) == 0) red[t >> 6] = acc;
    __syncthreads();
    if (t == 0) partial[c] = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();                              // red is written again on the block's next trip
  }
}

// Graph-replayable AdamW: step count and hyper-parameters live in device memory, so a captured
// launch picks up the next step's bias correction and a scheduler's new lr on every replay.
// hyper = {lr, beta1, beta2, eps, weight_decay, grad_scale}; state = {step, bc1, 1/sqrt(bc2)}
__device__ __forceinline__ void adam_tick(float* state, const float* hyper) {
  const double step = (double)state[0] + 1.0;
  state[0] = (float)step;
  state[1] = (float)(1.0 - pow((double)hyper[1], step));
  state[2] = (float)(1.0 / sqrt(1.0 - pow((double)hyper[2], step)));
}
__global__ void adam_tick_kernel(float* state, const float* hyper) {
  if (threadIdx.x == 0 && blockIdx.x == 0) adam_tick(state, hyper);
}

// clipcfg = {max_norm, skip_nonfinite}; clip = {norm, coef, finite, skipped_total}
__global__ __launch_bounds__(256) void grad_clip_finalize_kernel(const double* __restrict__ partial, int nchunks,
                                                                 const float* __restrict__ hyper,
                                                                 const float* __restrict__ clipcfg, float* state,
                                                                 float* clip) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  double acc = 0.0;
  for (int i = t; i < nchunks; i += 256) acc += partial[i];
  acc = wave_sum_d(acc);
  if ((t & 63) == 0) red[t >> 6] = acc;
  __syncthreads();
  if (t != 0) return;
  const double S = ((red[0] + red[1]) + red[2]) + red[3];
  const double s = (double)hyper[5];
  const double norm = fabs(s) * sqrt(S);
  const bool finite = isfinite(S) && isfinite(s);
  // torch.nn.utils.clip_grad_norm_ (norm_type 2): clamp(max_norm / (norm + 1e-6), max=1.0); a NaN quotient stays NaN
  const double q = (double)clipcfg[0] / (norm + 1e-6);
  const double coef = (q > 1.0) ? 1.0 : q;
  const bool is_void = (clipcfg[1] != 0.f) && !finite;
  clip[0] = (float)norm;
  clip[1] = (float)coef;
  clip[2] = finite ? 1.f : 0.f;
  if (is_void) {
    clip[3] = clip[3] + 1.f;
  } else {
    adam_tick(state, hyper);
  }
}

// emacfg = {decay, warmup (0 or 1), s0}; state[0] = s, the step count AFTER this step's tick.  t = s - s0 - 1 updates of
// the shadow have been done; eff = warmup ? min(d, (1 + t) / (10 + t)) : d; -> alpha = 1 - eff.  All counts are small
// integers held exactly in fp32.  Evaluated once per thread from grid-uniform scalars.
__device__ __forceinline__ float ema_alpha(const float* __restrict__ state, const float* __restrict__ emacfg) {
  const float d = emacfg[0], t = state[0] - emacfg[2] - 1.f;
  const float eff = (emacfg[1] != 0.f) ? fminf(d, (1.f + t) / (10.f + t)) : d;
  return 1.f - eff;
}
// e + (p' - e) * alpha, the product and the sum as ONE fused multiply-add -- spelled out, so that the fused update
// kernels and ema_update_kernel round alike whatever the compiler would contract on its own.
__device__ __forceinline__ float ema_line(float e, float p, float alpha) { return __builtin_fmaf(p - e, alpha, e); }

// AdamW over one flat buffer (torch.optim.AdamW single-tensor semantics; step = lr / bc1).  CLIP = true scales the gradient
// by coef as well; a step whose coef is exactly 1 takes CLIP = false and so rounds exactly as the plain update does.  EMA = true
// appends the shadow's update on the p' just computed (still in its registers); p, m, v are computed and stored as with EMA = false.
template <bool CLIP, bool EMA = false>
__device__ __forceinline__ void adamw_body(float* __restrict__ p, const float* __restrict__ g,
                                                float* __restrict__ m, float* __restrict__ v, long n4, long n, float lr,
                                                float b1, float b2, float eps, float wd, float gscale, float coef,
                                                float step, float rsqrt_bc2, float* __restrict__ e = nullptr,
                                                float alpha = 0.f) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    f32x4 pp = ld4(p + 4 * i), gg = ld4(g + 4 * i) * gscale, mm = ld4(m + 4 * i), vv = ld4(v + 4 * i);
    if (CLIP) gg = gg * coef;
    pp = pp * (1.f - lr * wd);
    mm = mm + (gg - mm) * (1.f - b1);          // lerp, as torch: m.lerp_(g, 1-b1)
    vv = vv * b2 + gg * gg * (1.f - b2);
#pragma unroll
    for (int j = 0; j < 4; ++j) pp[j] -= step * mm[j] / (sqrtf(vv[j]) * rsqrt_bc2 + eps);
    st4(p + 4 * i, pp);
    st4(m + 4 * i, mm);
    st4(v + 4 * i, vv);
    if (EMA) {
      f32x4 ee = ld4(e + 4 * i);
#pragma unroll
      for (int j = 0; j < 4; ++j) ee[j] = ema_line(ee[j], pp[j], alpha);
      st4(e + 4 * i, ee);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n - 4 * n4)) {  // tail
    const long i = 4 * n4 + threadIdx.x;
    float pp = p[i] * (1.f - lr * wd), gg = g[i] * gscale;
    if (CLIP) gg = gg * coef;
    const float mm = m[i] + (gg - m[i]) * (1.f - b1), vv = v[i] * b2 + gg * gg * (1.f - b2);
    if (EMA) {
      pp = pp - step * mm / (sqrtf(vv) * rsqrt_bc2 + eps);
      p[i] = pp;
      e[i] = ema_line(e[i], pp, alpha);
    } else {
      p[i] = pp - step * mm / (sqrtf(vv) * rsqrt_bc2 + eps);
    }
    m[i] = mm;
    v[i] = vv;
  }
}

// host scalars
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v, long n4, long n,
                                                    float lr, float b1, float b2, float eps, float wd, float bc1,
                                                    float rsqrt_bc2, float gscale) {
  adamw_body<false>(p, g, m, v, n4, n, lr, b1, b2, eps, wd, gscale, 1.f, lr / bc1, rsqrt_bc2);
}

__global__ __launch_bounds__(256) void adamw_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v, long n4, long n,
                                                        const float* __restrict__ hyper,
                                                        const float* __restrict__ state) {
  const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], wd = hyper[4], gscale = hyper[5];
  const float step = lr / state[1], rsqrt_bc2 = state[2];
  // adamw_body<false>, written out.  Built on the template this kernel -- the one every default training step launches -- reads
  // blockDim with a vector load from the dispatch packet ahead of its loop (as the clip / EMA kernels do) instead of a scalar
  // load of the kernel arguments: 6 instructions more, same loop.  Measured on MI355X, medians of three alternating runs, us per
  // call: 65.9 M elements 318.2 -> 321.4 (parent's own spread 4.2), 13.4 M elements 60.14 -> 60.81 (spread 0.48): outside the
  // spread at the smaller size and above the parent in every pair, so the step's kernel keeps its own text.
  // tests/test_gradclip_gpu.py holds the two spellings together bit for bit (adamw_dev against adamw_dev_clip at coef == 1).
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    f32x4 pp = ld4(p + 4 * i), gg = ld4(g + 4 * i) * gscale, mm = ld4(m + 4 * i), vv = ld4(v + 4 * i);
    pp = pp * (1.f - lr * wd);
    mm = mm + (gg - mm) * (1.f - b1);
    vv = vv * b2 + gg * gg * (1.f - b2);
#pragma unroll
    for (int j = 0; j < 4; ++j) pp[j] -= step * mm[j] / (sqrtf(vv[j]) * rsqrt_bc2 + eps);
    st4(p + 4 * i, pp);
    st4(m + 4 * i, mm);
    st4(v + 4 * i, vv);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n - 4 * n4)) {
    const long i = 4 * n4 + threadIdx.x;
    float pp = p[i] * (1.f - lr * wd), gg = g[i] * gscale;
    const float mm = m[i] + (gg - m[i]) * (1.f - b1), vv = v[i] * b2 + gg * gg * (1.f - b2);
    p[i] = pp - step * mm / (sqrtf(vv) * rsqrt_bc2 + eps);
    m[i] = mm;
    v[i] = vv;
  }
}

__global__ __launch_bounds__(256) void adamw_dev_clip_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                             float* __restrict__ m, float* __restrict__ v, long n4, long n,
                                                             const float* __restrict__ hyper,
                                                             const float* __restrict__ state,
                                                             const float* __restrict__ clipcfg,
                                                             const float* __restrict__ clip) {
  if (clipcfg[1] != 0.f && clip[2] == 0.f) return;      // void step: p, m, v stay as they are (grid-uniform)
  const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], wd = hyper[4], gscale = hyper[5];
  const float step = lr / state[1], rsqrt_bc2 = state[2], coef = clip[1];
  if (coef == 1.f) adamw_body<false>(p, g, m, v, n4, n, lr, b1, b2, eps, wd, gscale, coef, step, rsqrt_bc2);
  else adamw_body<true>(p, g, m, v, n4, n, lr, b1, b2, eps, wd, gscale, coef, step, rsqrt_bc2);
}

// --------------------------------------------------------------------------- weight EMA
__global__ __launch_bounds__(256) void adamw_dev_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                            float* __restrict__ m, float* __restrict__ v,
                                                            float* __restrict__ e, long n4, long n,
                                                            const float* __restrict__ hyper,
                                                            const float* __restrict__ state,
                                                            const float* __restrict__ emacfg) {
  const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], wd = hyper[4], gscale = hyper[5];
  const float step = lr / state[1], rsqrt_bc2 = state[2];
  adamw_body<false, true>(p, g, m, v, n4, n, lr, b1, b2, eps, wd, gscale, 1.f, step, rsqrt_bc2, e,
                               ema_alpha(state, emacfg));
}

__global__ __launch_bounds__(256) void adamw_dev_clip_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                 float* __restrict__ m, float* __restrict__ v,
                                                                 float* __restrict__ e, long n4, long n,
                                                                 const float* __restrict__ hyper,
                                                                 const float* __restrict__ state,
                                                                 const float* __restrict__ clipcfg,
                                                                 const float* __restrict__ clip,
                                                                 const float* __restrict__ emacfg) {
  if (clipcfg[1] != 0.f && clip[2] == 0.f) return;      // void step: p, m, v AND e stay as they are (grid-uniform)
  const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], wd = hyper[4], gscale = hyper[5];
  const float step = lr / state[1], rsqrt_bc2 = state[2], coef = clip[1];
  const float alpha = ema_alpha(state, emacfg);
  if (coef == 1.f) adamw_body<false, true>(p, g, m, v, n4, n, lr, b1, b2, eps, wd, gscale, coef, step, rsqrt_bc2, e, alpha);
  else adamw_body<true, true>(p, g, m, v, n4, n, lr, b1, b2, eps, wd, gscale, coef, step, rsqrt_bc2, e, alpha);
}

// the shadow's update alone, for a p that has its step behind it (state already advanced)
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ e, const float* __restrict__ p, long n4, long n,
                                                         const float* __restrict__ state,
                                                         const float* __restrict__ emacfg) {
  const float alpha = ema_alpha(state, emacfg);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    f32x4 ee = ld4(e + 4 * i);
    const f32x4 pp = ld4(p + 4 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j) ee[j] = ema_line(ee[j], pp[j], alpha);
    st4(e + 4 * i, ee);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n - 4 * n4)) {
    const long i = 4 * n4 + threadIdx.x;
    e[i] = ema_line(e[i], p[i], alpha);
  }
}

// a <-> b, contents not pointers: whoever holds either address (a recorded launch tape) keeps a valid one
__global__ __launch_bounds__(256) void swap_kernel(float* __restrict__ a, float* __restrict__ b, long n4, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const f32x4 aa = ld4(a + 4 * i), bb = ld4(b + 4 * i);
    st4(a + 4 * i, bb);
    st4(b + 4 * i, aa);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n - 4 * n4)) {
    const long i = 4 * n4 + threadIdx.x;
    const float aa = a[i], bb = b[i];
    a[i] = bb;
    b[i] = aa;
  }
}

__global__ void fill_kernel(float* p, float v, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = v;
}

// --------------------------------------------------------------------------- entry points
extern "C" int hrseg_fill(float* p, float v, long n, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(p && n >= 0, "hrseg_fill: bad arguments");
  if (n == 0) return 0;
  long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(fill_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, p, v, n);
  HRSEG_LAUNCH_CHECK("fill");
  return 0;
}

extern "C" int hrseg_adamw(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                           float eps, float weight_decay, float bc1, float bc2, float gscale,
                           hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(p && g && m && v && n > 0, "hrseg_adamw: bad arguments");
  HRSEG_CHECK_ARG(al16(p) && al16(g) && al16(m) && al16(v), "hrseg_adamw: buffers must be 16-byte aligned");
  const long n4 = n / 4;
  hipLaunchKernelGGL(adamw_kernel, dim3(flat_blocks(n4)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n4, n, lr, beta1,
                     beta2, eps, weight_decay, bc1, 1.0f / sqrtf(bc2), gscale);
  HRSEG_LAUNCH_CHECK("adamw");
  return 0;
}

extern "C" int hrseg_adamw_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, float* state,
                               hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(p && g && m && v && hyper && state && n > 0, "hrseg_adamw_dev: bad arguments");
  HRSEG_CHECK_ARG(al16(p) && al16(g) && al16(m) && al16(v), "hrseg_adamw_dev: buffers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(64), 0, st, state, hyper);
  HRSEG_LAUNCH_CHECK("adam_tick");
  const long n4 = n / 4;
  hipLaunchKernelGGL(adamw_dev_kernel, dim3(flat_blocks(n4)), dim3(256), 0, st, p, g, m, v, n4, n, hyper, state);
  HRSEG_LAUNCH_CHECK("adamw_dev");
  return 0;
}

extern "C" int hrseg_grad_sumsq_chunk_len(void) { return GRAD_CHUNK; }
extern "C" int hrseg_grad_sumsq_max_blocks(void) { return GRAD_MAX_BLOCKS; }

extern "C" int hrseg_grad_sumsq_chunks(long n) {
  HRSEG_CHECK_ARG(n > 0 && (n + GRAD_CHUNK - 1) / GRAD_CHUNK <= 0x7fffffffL, "hrseg_grad_sumsq_chunks: n=%ld out of range", n);
  return (int)((n + GRAD_CHUNK - 1) / GRAD_CHUNK);
}

extern "C" int hrseg_grad_sumsq(const float* g, long n, double* partial, int nchunks, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(g && partial && n > 0, "hrseg_grad_sumsq: bad arguments");
  HRSEG_CHECK_ARG(al16(g) && ((uintptr_t)partial % 8 == 0), "hrseg_grad_sumsq: g must be 16-byte aligned, partial 8-byte aligned");
  HRSEG_CHECK_ARG(hrseg_grad_sumsq_chunks(n) == nchunks, "hrseg_grad_sumsq: nchunks=%d does not match n=%ld (%ld per chunk)",
                  nchunks, n, (long)GRAD_CHUNK);
  const int blocks = nchunks < GRAD_MAX_BLOCKS ? nchunks : GRAD_MAX_BLOCKS;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, n, partial, nchunks);
  HRSEG_LAUNCH_CHECK("grad_sumsq");
  return 0;
}

extern "C" int hrseg_grad_clip_finalize(const double* partial, int nchunks, const float* hyper, const float* clipcfg,
                                        float* state, float* clip, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(partial && hyper && clipcfg && state && clip && nchunks > 0, "hrseg_grad_clip_finalize: bad arguments");
  HRSEG_CHECK_ARG((uintptr_t)partial % 8 == 0, "hrseg_grad_clip_finalize: partial must be 8-byte aligned");
  hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, nchunks, hyper, clipcfg,
                     state, clip);
  HRSEG_LAUNCH_CHECK("grad_clip_finalize");
  return 0;
}

extern "C" int hrseg_adamw_dev_clip(float* p, const float* g, float* m, float* v, long n, const float* hyper,
                                    const float* state, const float* clipcfg, const float* clip, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(p && g && m && v && hyper && state && clipcfg && clip && n > 0, "hrseg_adamw_dev_clip: bad arguments");
  HRSEG_CHECK_ARG(al16(p) && al16(g) && al16(m) && al16(v), "hrseg_adamw_dev_clip: buffers must be 16-byte aligned");
  const long n4 = n / 4;
  hipLaunchKernelGGL(adamw_dev_clip_kernel, dim3(flat_blocks(n4)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n4, n, hyper,
                     state, clipcfg, clip);
  HRSEG_LAUNCH_CHECK("adamw_dev_clip");
  return 0;
}

extern "C" int hrseg_adamw_dev_ema(float* p, const float* g, float* m, float* v, float* e, long n, const float* hyper,
                                   float* state, const float* emacfg, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(p && g && m && v && e && hyper && state && emacfg && n > 0, "hrseg_adamw_dev_ema: bad arguments");
  HRSEG_CHECK_ARG(al16(p) && al16(g) && al16(m) && al16(v) && al16(e), "hrseg_adamw_dev_ema: buffers must be 16-byte aligned");
  HRSEG_CHECK_ARG(e != p && e != g && e != m && e != v, "hrseg_adamw_dev_ema: the shadow must be a buffer of its own");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(64), 0, st, state, hyper);
  HRSEG_LAUNCH_CHECK("adam_tick");
  const long n4 = n / 4;
  hipLaunchKernelGGL(adamw_dev_ema_kernel, dim3(flat_blocks(n4)), dim3(256), 0, st, p, g, m, v, e, n4, n, hyper, state, emacfg);
  HRSEG_LAUNCH_CHECK("adamw_dev_ema");
  return 0;
}

extern "C" int hrseg_adamw_dev_clip_ema(float* p, const float* g, float* m, float* v, float* e, long n, const float* hyper,
                                        const float* state, const float* clipcfg, const float* clip, const float* emacfg,
                                        hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(p && g && m && v && e && hyper && state && clipcfg && clip && emacfg && n > 0,
                  "hrseg_adamw_dev_clip_ema: bad arguments");
  HRSEG_CHECK_ARG(al16(p) && al16(g) && al16(m) && al16(v) && al16(e),
                  "hrseg_adamw_dev_clip_ema: buffers must be 16-byte aligned");
  HRSEG_CHECK_ARG(e != p && e != g && e != m && e != v, "hrseg_adamw_dev_clip_ema: the shadow must be a buffer of its own");
  const long n4 = n / 4;
  hipLaunchKernelGGL(adamw_dev_clip_ema_kernel, dim3(flat_blocks(n4)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, e, n4, n,
                     hyper, state, clipcfg, clip, emacfg);
  HRSEG_LAUNCH_CHECK("adamw_dev_clip_ema");
  return 0;
}

extern "C" int hrseg_ema_update(float* e, const float* p, long n, const float* state, const float* emacfg,
                                hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(e && p && state && emacfg && n > 0, "hrseg_ema_update: bad arguments");
  HRSEG_CHECK_ARG(al16(e) && al16(p), "hrseg_ema_update: buffers must be 16-byte aligned");
  HRSEG_CHECK_ARG(e != p, "hrseg_ema_update: the shadow must be a buffer of its own");
  const long n4 = n / 4;
  hipLaunchKernelGGL(ema_update_kernel, dim3(flat_blocks(n4)), dim3(256), 0, (hipStream_t)stream, e, p, n4, n, state, emacfg);
  HRSEG_LAUNCH_CHECK("ema_update");
  return 0;
}

extern "C" int hrseg_swap(float* a, float* b, long n, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(a && b && n > 0, "hrseg_swap: bad arguments");
  HRSEG_CHECK_ARG(al16(a) && al16(b), "hrseg_swap: buffers must be 16-byte aligned");
  HRSEG_CHECK_ARG(a + n <= b || b + n <= a, "hrseg_swap: the buffers overlap");
  const long n4 = n / 4;
  hipLaunchKernelGGL(swap_kernel, dim3(flat_blocks(n4)), dim3(256), 0, (hipStream_t)stream, a, b, n4, n);
  HRSEG_LAUNCH_CHECK("swap");
  return 0;
}
