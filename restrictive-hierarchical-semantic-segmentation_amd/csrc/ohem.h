// Online hard example mining, the part loss.hip (masked loss instances) and loss_ohem.hip (scores, selection) share: the
// 16-byte device record of a selection, the keep rule and the checks on the options.  DESIGN.md section 18.
#pragma once
#include <cfloat>

// what hrseg_ohem_select leaves on the device (hrseg.h): lam_k = the min(min_kept, N)-th smallest candidate score, -1 when
// min_kept = 0 or there is no candidate; n_candidates = N; n_kept = candidates the rule below keeps
struct OhemRecord {
  float lam_k;
  int n_candidates, n_kept, reserved;
};
static_assert(sizeof(OhemRecord) == 16, "the record is 16 bytes in hrseg.h");

// A candidate (score != -1) is kept iff its score is NaN, below thresh, or not above lam_k.  Forward, backward and the
// selection's own count take the decision from the STORED score through this one expression.  Non-candidates carry -1: they
// pass it (any thresh >= 0 is above -1), and have no valid channel for it to matter.
__device__ __forceinline__ bool ohem_kept(float q, float thresh, float lam_k) { return q != q || q < thresh || q <= lam_k; }

static inline bool ohem_thresh_ok(float v) { return v >= 0.f && v <= 1.f; }       // (false for NaN)
