// What the two producers of target planes (targets.hip, augment.hip) share: the parent table as a kernel argument and the
// rule that turns a pixel's node sets into the ternary channel values.  Semantics: include/hrseg.h, "partial labels".
#pragma once

struct TargetParents { int parent[64]; };

// host: the table of a C-channel call; returns the first channel whose parent is outside -1..C-1, or -1
static inline int target_parents(const int* parent, int C, TargetParents& pr) {
  for (int c = 0; c < 64; ++c) pr.parent[c] = -1;
  for (int c = 0; c < C; ++c) {
    if (parent[c] < -1 || parent[c] >= C) return c;
    pr.parent[c] = parent[c];
  }
  return -1;
}

// channel c of a pixel with the sets (on, unk): 1 on the node; else -1 where the node is unknown; else 0 for a root or inside
// the direct parent's area; else -1 (outside the parent: ignored by loss and metrics).  unk == 0 is the rule of fully
// labelled maps.
__device__ __forceinline__ void encode_write(unsigned long long on, unsigned long long unk, const TargetParents& pr,
                                             float* __restrict__ o, int C, size_t plane) {
  for (int c = 0; c < C; ++c) {
    const int par = pr.parent[c];
    float v;
    if ((on >> c) & 1ull) v = 1.f;
    else if ((unk >> c) & 1ull) v = -1.f;
    else if (par < 0 || ((on >> par) & 1ull)) v = 0.f;
    else v = -1.f;
    o[(size_t)c * plane] = v;
  }
}
