// What the units that work on ragged uint8 label maps share (score.hip, components.hip, boundary.hip, instances.hip,
// calibration.hip, decode_hedged.hip; the decode units get the typedefs through decode_common.h): the integer typedefs,
// the wave-folded LDS add, the rule that decides whether a path_lut entry is a leaf, the int wave reductions and, on the
// host, the check of one row of a host descriptor table and of the sizes of a [2][B][4] pair of tables.  Only what at
// least two units use lives here.  NOT here, on purpose: the level-table checks, and the device
// descriptor readers (cc_image, in_image, bd_image, ...), whose acceptance rules differ at the edges as hrseg.h states.
#pragma once
#include "common.h"

typedef unsigned char u8;
typedef unsigned u32;
typedef unsigned long long u64;

// ---- the wave-folded LDS add.  Real maps are dominated by one value (background on background), so most lanes of a wave
// hold the same key.  Inside a call every participating lane holds one key and the same count: the wave elects the first
// such lane, ballots the lanes with the same key and the leader adds count * popcount once; after LM_PEEL such rounds
// the lanes that are left (many distinct keys: a noisy map) add for themselves.
// Two leader loops of the same shape stay where they are because they are different loops:
//   bd_mark_kernel (boundary.hip): unbounded, and the ballot of a round is written out as bitmap words, not added;
//   cc_flatten_kernel (components.hip): the lanes of a key hold unequal counts, so a round sums them (lm_wave_sum).
#define LM_PEEL 4
// every lane with `has` adds `cnt` (the same in all of them) to cells[key]; called by whole waves
__device__ __forceinline__ void lm_wave_add(unsigned* cells, unsigned key, unsigned cnt, bool has, int lane) {
  u64 todo = __ballot(has);
  for (int it = 0; it < LM_PEEL && todo; ++it) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned k = (unsigned)__builtin_amdgcn_readlane((int)key, leader);
    const bool same = has && key == k;
    const u64 m = __ballot(same);
    if (lane == leader) atomicAdd(&cells[k], cnt * (unsigned)__popcll(m));
    has = has && !same;
    todo &= ~m;
  }
  if (has) atomicAdd(&cells[key], cnt);
}

__device__ __forceinline__ int lm_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int lm_wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- a path_lut entry.  path_lut[v] is the path of pixel value v down the class tree, one byte per level: byte L is
// 1 + the channel at level L, 0 below the path's end; the whole entry 0 = v is no leaf's value.  An entry counts as "no
// leaf" (e = 0) when it has no level-0 node, names a channel outside its level, or has a byte at or above `nlevels`.
// LM_PATH_ENTRY(e, a) applies that to the u64 lvalue e with a.nlevels and a.C[] of the kernel's own argument struct.  A
// statement macro, not a function: handing a member of the by-value kernel argument to a function (pointer, reference or
// copy) changed the code of all three kernels that use it.  ops.check_score_tables is the host
// (Python) statement of the same rule.
static_assert(HRSEG_SCORE_MAX_LEVELS == HRSEG_DECODE_MAX_LEVELS, "one path format for the scoring and the decode tables");
#define LM_PATH_ENTRY(e, a)                                                              \
  {                                                                                      \
    bool ok = e != 0;                                                                    \
    _Pragma("unroll") for (int L = 0; L < HRSEG_SCORE_MAX_LEVELS; ++L) {                 \
      const int c = (int)((e >> (8 * L)) & 0xffu);                                       \
      if (L >= a.nlevels ? c != 0 : (c > a.C[L] || (L == 0 && c == 0))) ok = false;      \
    }                                                                                    \
    if (!ok) e = 0;                                                                      \
  }

// ---- host: one row of a host descriptor table (offset, H, W, channels).  `who` is the entry point's name, `what` goes in
// front of "image" ("predicted " / "ground-truth " where an entry point reads two tables, "" otherwise).
static inline int lm_host_image(const char* who, const char* what, const long* desc_host, int b, long long* off, long long* H,
                                long long* W) {
  const long long ch = desc_host[4 * b + 3];
  *off = desc_host[4 * b], *H = desc_host[4 * b + 1], *W = desc_host[4 * b + 2];
  HRSEG_CHECK_ARG(*off >= 0 && *H >= 1 && *W >= 1 && ch == 1, "%s: %simage %d: bad descriptor (offset %lld, %lld x %lld, %lld channels)",
                  who, what, b, *off, *H, *W, ch);
  HRSEG_CHECK_ARG(*H <= ((1ll << 31) - 1) / *W, "%s: %simage %d: %lld x %lld has 2^31 pixels or more", who, what, b, *H, *W);
  return 0;
}

// the two halves of a [2][B][4] host table (predictions, then ground truth) agree on every size
static inline int lm_host_same_sizes(const char* who, const long* desc_host, int B) {
  for (int b = 0; b < B; ++b) {
    const long* p = desc_host + 4 * (size_t)b;
    const long* g = p + 4 * (size_t)B;
    HRSEG_CHECK_ARG(p[1] == g[1] && p[2] == g[2], "%s: image %d: predicted map %ld x %ld, ground truth %ld x %ld", who, b, p[1], p[2], g[1],
                    g[2]);
  }
  return 0;
}
