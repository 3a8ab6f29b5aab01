// Phase stamps for the halo-patch conv kernel (diagnostic build; read the shares).
#include "../../restrictive-hierarchical-semantic-segmentation_amd/csrc/runtime.hip"
#include "../../restrictive-hierarchical-semantic-segmentation_amd/csrc/conv.hip"
#include <vector>
#include <algorithm>
#include <stdlib.h>
__device__ __forceinline__ unsigned long long stamp() {
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
template <int TH, int WTN>
__global__ __launch_bounds__(256) void patch_stamped(PatchArgs p, unsigned long long* prof) {
  constexpr int BN = 16 * WTN, PW = 18, PROWS = (TH + 2) * PW, PSTR = 20;
  constexpr int P_F4 = PROWS * 4, W_F4 = BN * 9 * 4;
  constexpr int P_LOADS = (P_F4 + 255) / 256, W_LOADS = (W_F4 + 255) / 256;
  constexpr int RPW = TH / 4;
  constexpr int KP = (RPW * WTN <= 3) ? 4 : (RPW * WTN <= 6) ? 2 : 1;
  __shared__ __attribute__((aligned(16))) float lds[PROWS * PSTR + BN * 9 * 16];
  float* lp = lds; float* lw = lds + PROWS * PSTR;
  const unsigned long long T0 = stamp();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ntn = p.N / BN;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int nt = wg % ntn; int mt = wg / ntn;
  const int tx = mt % p.tiles_x; mt /= p.tiles_x;
  const int ty = mt % p.tiles_y, b = mt / p.tiles_y;
  const int y0 = ty * TH, x0 = tx * 16, n0 = nt * BN;
  long p_off[P_LOADS]; int p_st[P_LOADS];
  for (int i = 0; i < P_LOADS; ++i) { const int f = tid + 256 * i; const int r = f >> 2, q = f & 3; const int py = r / PW, px = r - py * PW;
    const int iy = y0 - 1 + py, ix = x0 - 1 + px; const bool ok = (f < P_F4) & (iy >= 0) & (iy < p.H) & (ix >= 0) & (ix < p.W);
    p_off[i] = ok ? ((long)(b * p.H + iy) * p.W + ix) * p.ldx + 4 * q : -1; p_st[i] = (f < P_F4) ? r * PSTR + 4 * q : -1; }
  long w_off[W_LOADS]; int w_st[W_LOADS];
  for (int i = 0; i < W_LOADS; ++i) { const int f = tid + 256 * i; const int r = f >> 2, q = f & 3; const int tap = r / BN, n = r - tap * BN;
    w_off[i] = (f < W_F4) ? ((long)(n0 + n) * 9 + tap) * p.K + 4 * q : -1; w_st[i] = (f < W_F4) ? r * 16 + 4 * lds_slot(n, q) : -1; }
  f32x4 rp[P_LOADS], rw[W_LOADS];
  auto stage_load = [&](int c0) {
    for (int i = 0; i < P_LOADS; ++i) { f32x4 v = {0.f, 0.f, 0.f, 0.f}; if (p_off[i] >= 0) v = *reinterpret_cast<const f32x4*>(p.x + p_off[i] + c0); rp[i] = v; }
    for (int i = 0; i < W_LOADS; ++i) { f32x4 v = {0.f, 0.f, 0.f, 0.f}; if (w_off[i] >= 0) v = *reinterpret_cast<const f32x4*>(p.w + w_off[i] + c0); rw[i] = v; } };
  auto stage_store = [&]() {
    for (int i = 0; i < P_LOADS; ++i) if (p_st[i] >= 0) *reinterpret_cast<f32x4*>(lp + p_st[i]) = rp[i];
    for (int i = 0; i < W_LOADS; ++i) if (w_st[i] >= 0) *reinterpret_cast<f32x4*>(lw + w_st[i]) = rw[i]; };
  f32x4 acc[KP][WTN][RPW];
  for (int kp = 0; kp < KP; ++kp) for (int n = 0; n < WTN; ++n) for (int m = 0; m < RPW; ++m) acc[kp][n][m] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int fi = lane & 15, fh = lane >> 4;
  const int woff = fi * 16 + 4 * lds_slot(fi, fh);
  const int nchunks = p.K >> 4;
  const unsigned long long T1 = stamp();
  stage_load(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned long long T2 = stamp();
  stage_store();
  __syncthreads();
  const unsigned long long T3 = stamp();
  unsigned long long ph[4] = {0, 0, 0, 0};
  for (int c = 0; c < nchunks; ++c) {
    const bool more = c + 1 < nchunks;
    unsigned long long t0 = stamp();
    if (more) stage_load((c + 1) << 4);
    __builtin_amdgcn_sched_barrier(0);
    unsigned long long t1 = stamp();
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int kh = t / 3, kw = t - 3 * kh;
      f32x4 xf[RPW], wf[WTN];
      for (int m = 0; m < RPW; ++m) xf[m] = *reinterpret_cast<const f32x4*>(lp + ((wave * RPW + m + kh) * PW + kw + fi) * PSTR + 4 * fh);
      for (int n = 0; n < WTN; ++n) wf[n] = *reinterpret_cast<const f32x4*>(lw + (t * BN + 16 * n) * 16 + woff);
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int n = 0; n < WTN; ++n)
#pragma unroll
          for (int m = 0; m < RPW; ++m) acc[k % KP][n][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[n][k], xf[m][k], acc[k % KP][n][m], 0, 0, 0);
    }
    asm volatile("" ::"v"(acc[0][0][0][0]), "v"(acc[KP - 1][WTN - 1][RPW - 1][0]));
    __builtin_amdgcn_sched_barrier(0);
    unsigned long long t2 = stamp();
    __syncthreads();
    unsigned long long t3 = stamp();
    if (more) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stage_store(); }
    __syncthreads();
    unsigned long long t4 = stamp();
    ph[0] += t1 - t0; ph[1] += t2 - t1; ph[2] += t3 - t2; ph[3] += t4 - t3;
  }
  const unsigned long long T4 = stamp();
  for (int m = 0; m < RPW; ++m) {
    const int oy = y0 + wave * RPW + m, ox = x0 + fi;
    if (oy >= p.H || ox >= p.W) continue;
    float* yrow = p.y + ((size_t)(b * p.H + oy) * p.W + ox) * p.ldy;
    for (int n = 0; n < WTN; ++n) { f32x4 v = acc[0][n][m]; for (int kp = 1; kp < KP; ++kp) v += acc[kp][n][m]; *reinterpret_cast<f32x4*>(yrow + n0 + 16 * n + 4 * fh) = v; }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned long long T5 = stamp();
  if (lane == 0) { unsigned long long* o = prof + ((size_t)blockIdx.x * 4 + wave) * 12;
    o[0] = T1 - T0; o[1] = T2 - T1; o[2] = T3 - T2; o[3] = ph[0]; o[4] = ph[1]; o[5] = ph[2]; o[6] = ph[3]; o[7] = T5 - T4; o[8] = T5 - T0; o[9] = T0; o[10] = T5; }
}
int main(int argc, char** argv) {
  const int B = 4, H = argc > 1 ? atoi(argv[1]) : 155, C = argc > 2 ? atoi(argv[2]) : 48;
  hrseg_conv_shape_t s{B, H, H, C, C, H, H, C, C, 3, 1};
  const size_t nx = (size_t)B * H * H * C, nw = (size_t)C * 9 * C;
  std::vector<float> hx(nx), hw(nw);
  for (auto& v : hx) v = (rand() % 2001 - 1000) * 1e-3f;
  for (auto& v : hw) v = (rand() % 2001 - 1000) * 5e-5f;
  float *x, *w, *y; unsigned long long* prof;
  (void)hipMalloc(&x, nx * 4); (void)hipMalloc(&w, nw * 4); (void)hipMalloc(&y, nx * 4);
  (void)hipMemcpy(x, hx.data(), nx * 4, hipMemcpyHostToDevice); (void)hipMemcpy(w, hw.data(), nw * 4, hipMemcpyHostToDevice);
  PatchArgs p; p.x = x; p.w = w; p.bias = nullptr; p.y = y; p.ldx = C; p.ldy = C; p.B = B; p.H = H; p.W = H; p.K = C; p.N = C;
  p.tiles_x = ceil_div(H, 16); p.tiles_y = ceil_div(H, 8); p.flip = 0; p.accumulate = 0;
  const int nblk = B * p.tiles_x * p.tiles_y * (C / 48);
  (void)hipMalloc(&prof, (size_t)nblk * 4 * 12 * 8);
  hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  for (int rep = 0; rep < 3; ++rep) hipLaunchKernelGGL((patch_stamped<8, 3>), dim3(nblk), dim3(256), 0, 0, p, prof);
  (void)hipEventRecord(e0); for (int rep = 0; rep < 10; ++rep) hipLaunchKernelGGL((patch_stamped<8, 3>), dim3(nblk), dim3(256), 0, 0, p, prof); (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
  float ms; (void)hipEventElapsedTime(&ms, e0, e1); printf("stamped patch kernel: %.1f us, %d blocks\n", ms * 100, nblk);
  std::vector<unsigned long long> hp((size_t)nblk * 4 * 12);
  (void)hipMemcpy(hp.data(), prof, hp.size() * 8, hipMemcpyDeviceToHost);
  double tot[9] = {0}; unsigned long long tmin = ~0ull, tmax = 0;
  for (size_t i = 0; i < (size_t)nblk * 4; ++i) { for (int k = 0; k < 9; ++k) tot[k] += hp[i * 12 + k]; tmin = std::min(tmin, hp[i * 12 + 9]); tmax = std::max(tmax, hp[i * 12 + 10]); }
  const char* names[8] = {"setup (index math)", "first loads: issue + wait", "first LDS store + barrier", "issue next-stage loads (all stages)", "9 taps x 24 MFMA (all stages)", "barrier after compute", "vmcnt + LDS store + barrier", "epilogue stores"};
  for (int k = 0; k < 8; ++k) printf("  %-38s %8.0f cycles/wave  %5.1f%%\n", names[k], tot[k] / (nblk * 4.0), 100 * tot[k] / tot[8]);
  printf("  wave lifetime %.0f cycles; kernel span %.0f cycles\n", tot[8] / (nblk * 4.0), (double)(tmax - tmin));
  return 0;
}
