// Split-precision grouped launch whose problems run either the halo-patch or the im2col body: kernel instances + launcher.
#include "sp_im2col.h"
#include "sp_patch.h"

// grouped launch whose problems run either body (the parallel HRNet branches: the wide high-resolution
// branches take the halo-patch body, the small low-resolution ones the im2col body with split-K)
template <int NS, int WTM, int WTN, int CS, int FLIP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(sp_patch_min_waves(NS, WTN, CS), 2)))
void igemm_sp_pgroup_kernel(IgemmGroup grp) {
  constexpr int A = SpPatchLds<NS, 8, WTN, CS>::BYTES, B = SpLds<NS, WTN>::BYTES;
  __shared__ __attribute__((aligned(16))) unsigned char lds[A > B ? A : B];
  int gi = 0;
  while (gi + 1 < grp.n && (int)blockIdx.x >= grp.blk_end[gi]) ++gi;
  const int local = blockIdx.x - (gi ? grp.blk_end[gi - 1] : 0);
  const int tiles = grp.tiles[gi];
  if (grp.kind[gi]) igemm_patch_sp_body<NS, 8, WTN, CS, FLIP>(grp.a[gi], lds, local, 1 << 29, tiles);   // one tile per block
  else igemm_sp_body<NS, WTM, WTN>(grp.a[gi], lds, local % tiles, tiles, local / tiles, grp.ksplit[gi]);
}

// --------------------------------------------------------------------------- launchers
template <int NS>
static int launch_pgroup(const IgemmGroup& g, int wtm, int wtn, int cs, int flip, hipStream_t st) {
  const dim3 grid(g.blk_end[g.n - 1]);
#define SPP(M_, N_, C_) \
  if (wtm == M_ && wtn == N_ && cs == C_) { \
    if (flip) hipLaunchKernelGGL((igemm_sp_pgroup_kernel<NS, M_, N_, C_, 1>), grid, dim3(256), 0, st, g); \
    else hipLaunchKernelGGL((igemm_sp_pgroup_kernel<NS, M_, N_, C_, 0>), grid, dim3(256), 0, st, g); \
    return 0; }
  SPP(1, 3, 3) SPP(2, 3, 3) SPP(1, 4, 4) SPP(2, 4, 4)
#undef SPP
  return 1;
}
int launch_sp_pgroup_kernel(int ns, const IgemmGroup& g, int wtm, int wtn, int cs, int flip, hipStream_t st) {
  return ns == 4 ? launch_pgroup<4>(g, wtm, wtn, cs, flip, st) : ns == 3 ? launch_pgroup<3>(g, wtm, wtn, cs, flip, st)
       : ns == 2 ? launch_pgroup<2>(g, wtm, wtn, cs, flip, st) : launch_pgroup<1>(g, wtm, wtn, cs, flip, st);
}
