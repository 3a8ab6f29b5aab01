// Online hard example mining for the fused cross-entropy: the per-pixel score pass and the exact
// on-device selection of lam_k, the k-th smallest candidate score of a level's whole batch.  gfx950.  The masked instances of
// the loss kernels that read the scores and the record live with their templates in loss.hip.
//
// Selection = a radix select over an order-preserving 32-bit key of the fp32 score, 11 + 11 + 10 bits from the top: each pass
// histograms the keys that still match the prefix found so far (per-block LDS histogram, flushed with integer atomics, so the
// counts do not depend on the block order), a one-wave scan kernel between the passes picks the bin that holds the rank and
// the rank that remains inside it.  No sort, no host read, no floating-point atomic.
#include "common.h"
#include "level_common.h"
#include "ohem.h"

// workspace, in 32-bit words: the three histograms, then the state the passes hand on
enum { OH_H0 = 0, OH_H1 = 2048, OH_H2 = 4096, OH_STATE = 5120, OH_WORDS = 5128 };
enum { ST_NCAND = 0, ST_NLT, ST_NNAN, ST_PREFIX, ST_RANK, ST_ACTIVE, ST_BELOW };
#define OHEM_MAX_N 2147483647L        // the counts of the record are ints

// fp32 -> unsigned key with the order of the floats (negatives below positives); every NaN, of either sign, is the largest
// key: NaN sorts last, as in torch.sort
__device__ __forceinline__ unsigned ohem_key(float q) {
  if (q != q) return 0xFFFFFFFFu;
  const unsigned u = __float_as_uint(q);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ohem_unkey(unsigned k) {
  if (k == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// q[b*hw + i] = sum over the valid channels of t_c softmax(z)_c, -1 where no channel is valid.  The softmax is the one of
// loss_partials_kernel, expression by expression.
template <int CT>
__global__ __launch_bounds__(256) void ohem_scores_kernel(const float* __restrict__ z, const float* __restrict__ t,
                                                          float* __restrict__ q, int C, long hw, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long b = i / hw, pix = i - b * hw;
    const float* zb = z + (size_t)b * C * hw + pix;
    const float* tb = t + (size_t)b * C * hw + pix;
    float zz[CT], tt[CT];
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
      zz[c] = zz[c] - m;
      s += (c < C) ? expf(zz[c]) : 0.f;
    }
    const float inv = 1.f / s;
    bool candidate = false;
    float score = 0.f;
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C && tt[c] != -1.f) {
        candidate = true;
        score += tt[c] * (expf(zz[c]) * inv);
      }
    q[i] = candidate ? score : -1.f;
  }
}

__global__ void ohem_zero_kernel(unsigned* ws) {
  for (int i = threadIdx.x; i < OH_WORDS; i += blockDim.x) ws[i] = 0u;
}

// PASS 0: key bits 31..21 of every candidate (2048 bins), and the three counts the record needs: candidates, scores below
// thresh, NaN scores.  PASS 1: bits 20..10 of the keys whose top 11 bits are the prefix's.  PASS 2: bits 9..0 (1024 bins) of
// those whose top 22 are.
template <int PASS>
__global__ __launch_bounds__(256) void ohem_hist_kernel(const float* __restrict__ q, long n, float thresh, unsigned* ws) {
  constexpr int BINS = PASS == 2 ? 1024 : 2048;
  constexpr int BASE = PASS == 0 ? OH_H0 : PASS == 1 ? OH_H1 : OH_H2;
  __shared__ unsigned hist[BINS];
  __shared__ unsigned cnt[3];
  unsigned prefix = 0u;
  if (PASS > 0) {
    if (ws[OH_STATE + ST_ACTIVE] == 0u) return;       // (the same word for every thread of the grid)
    prefix = ws[OH_STATE + ST_PREFIX];
  }
  for (int i = threadIdx.x; i < BINS; i += 256) hist[i] = 0u;
  if (threadIdx.x < 3) cnt[threadIdx.x] = 0u;
  __syncthreads();
  unsigned ncand = 0u, nlt = 0u, nnan = 0u;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = q[i];
    if (v == -1.f) continue;
    const unsigned key = ohem_key(v);
    if (PASS == 0) {
      ++ncand;
      nlt += (v < thresh) ? 1u : 0u;
      nnan += (v != v) ? 1u : 0u;
      atomicAdd(&hist[key >> 21], 1u);
    } else if (PASS == 1) {
      if ((key >> 21) == (prefix >> 21)) atomicAdd(&hist[(key >> 10) & 2047u], 1u);
    } else {
      if ((key >> 10) == (prefix >> 10)) atomicAdd(&hist[key & 1023u], 1u);
    }
  }
  if (PASS == 0) {
    if (ncand) atomicAdd(&cnt[0], ncand);
    if (nlt) atomicAdd(&cnt[1], nlt);
    if (nnan) atomicAdd(&cnt[2], nnan);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < BINS; i += 256)
    if (hist[i]) atomicAdd(ws + BASE + i, hist[i]);
  if (PASS == 0 && threadIdx.x < 3 && cnt[threadIdx.x]) atomicAdd(ws + OH_STATE + threadIdx.x, cnt[threadIdx.x]);
}

// One wave.  Finds the bin of histogram PASS that holds the rank still looked for (lane l owns BINS/64 consecutive bins: chunk
// sums, a wave scan, then the owning lane walks its chunk) and hands prefix / remaining rank / keys below on.  PASS 0 first
// decides from min_kept and the candidate count whether there is a rank at all; PASS 2 writes the record.
template <int PASS>
__global__ __launch_bounds__(64) void ohem_scan_kernel(unsigned* ws, long min_kept, OhemRecord* __restrict__ rec) {
  constexpr int BINS = PASS == 2 ? 1024 : 2048;
  constexpr int BASE = PASS == 0 ? OH_H0 : PASS == 1 ? OH_H1 : OH_H2;
  constexpr int PER = BINS / 64;
  __shared__ unsigned h[BINS + BINS / 32];            // one pad word per 32 bins: the chunk walks of the lanes miss each other
  unsigned* st = ws + OH_STATE;
  const int lane = threadIdx.x;
  const unsigned ncand = st[ST_NCAND], nlt = st[ST_NLT], nnan = st[ST_NNAN];
  const unsigned prefix = st[ST_PREFIX], below0 = st[ST_BELOW];
  unsigned rank;
  if (PASS == 0) {
    if (min_kept < 1 || ncand == 0u) {                // no rank: lam_k = -1, the threshold alone decides
      if (lane == 0) {
        st[ST_ACTIVE] = 0u;
        rec->lam_k = -1.f;
        rec->n_candidates = (int)ncand;
        rec->n_kept = (int)(nlt + nnan);
        rec->reserved = 0;
      }
      return;
    }
    rank = min_kept < (long)ncand ? (unsigned)min_kept : ncand;
  } else {
    if (st[ST_ACTIVE] == 0u) return;
    rank = st[ST_RANK];
  }
  for (int i = lane; i < BINS; i += 64) h[i + (i >> 5)] = ws[BASE + i];
  __syncthreads();
  unsigned sum = 0u;
#pragma unroll 4
  for (int j = 0; j < PER; ++j) {
    const int i = lane * PER + j;
    sum += h[i + (i >> 5)];
  }
  unsigned incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  const unsigned long long has = __ballot(incl >= rank);
  const int owner = has ? __ffsll((long long)has) - 1 : 63;      // (the histogram holds at least `rank` keys: has != 0)
  if (lane != owner) return;
  unsigned below = incl - sum;
  int bin = lane * PER + PER - 1;
  for (int j = 0; j < PER; ++j) {
    const int i = lane * PER + j;
    const unsigned v = h[i + (i >> 5)];
    if (below + v >= rank) {
      bin = i;
      break;
    }
    if (j + 1 < PER) below += v;
  }
  if (PASS == 0) {
    st[ST_ACTIVE] = 1u;
    st[ST_PREFIX] = (unsigned)bin << 21;
    st[ST_RANK] = rank - below;
    st[ST_BELOW] = below;
  } else if (PASS == 1) {
    st[ST_PREFIX] = prefix | ((unsigned)bin << 10);
    st[ST_RANK] = rank - below;
    st[ST_BELOW] = below0 + below;
  } else {
    const unsigned key = prefix | (unsigned)bin;
    const unsigned equal = h[bin + (bin >> 5)];
    // scores <= lam_k: the keys below it and its ties.  Scores below thresh and scores <= lam_k are both lower sets of one
    // order, so their union is the larger of the two; NaN scores are kept on top (a NaN lam_k compares false with all)
    const unsigned nle = (key == 0xFFFFFFFFu) ? 0u : below0 + below + equal;
    rec->lam_k = ohem_unkey(key);
    rec->n_candidates = (int)ncand;
    rec->n_kept = (int)((nlt > nle ? nlt : nle) + nnan);
    rec->reserved = 0;
  }
}

extern "C" size_t hrseg_ohem_workspace_bytes(void) { return (size_t)OH_WORDS * sizeof(unsigned); }

extern "C" int hrseg_ohem_scores(const float* z, const float* t, float* q, int B, int C, long hw, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(z && t && q, "hrseg_ohem_scores: null pointer");
  HRSEG_CHECK_ARG(B > 0 && C > 0 && C <= MAXC && hw > 0 && hw <= OHEM_MAX_N / B, "hrseg_ohem_scores: bad arguments (B=%d C=%d hw=%ld)",
                  B, C, hw);
  hipStream_t st = (hipStream_t)stream;
  const long n = (long)B * hw;
  dim3 grid(pixel_blocks(n, 1L << 20));
  if (C <= 4) hipLaunchKernelGGL((ohem_scores_kernel<4>), grid, dim3(256), 0, st, z, t, q, C, hw, n);
  else if (C <= 8) hipLaunchKernelGGL((ohem_scores_kernel<8>), grid, dim3(256), 0, st, z, t, q, C, hw, n);
  else hipLaunchKernelGGL((ohem_scores_kernel<16>), grid, dim3(256), 0, st, z, t, q, C, hw, n);
  hrseg_count(CNT_OHEM);
  HRSEG_LAUNCH_CHECK("ohem_scores");
  return 0;
}

extern "C" int hrseg_ohem_select(const float* q, long n, float thresh, long min_kept, void* workspace, void* record,
                                 hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(q && workspace && record, "hrseg_ohem_select: null pointer");
  HRSEG_CHECK_ARG(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)record & 3) == 0, "hrseg_ohem_select: workspace and record must be 4-byte aligned");
  HRSEG_CHECK_ARG(n > 0 && n <= OHEM_MAX_N, "hrseg_ohem_select: n=%ld not in 1..%ld", n, OHEM_MAX_N);
  HRSEG_CHECK_ARG(ohem_thresh_ok(thresh), "hrseg_ohem_select: thresh must be a finite number in [0, 1] (got %g)", (double)thresh);
  HRSEG_CHECK_ARG(min_kept >= 0, "hrseg_ohem_select: min_kept must be >= 0 (got %ld)", min_kept);
  hipStream_t st = (hipStream_t)stream;
  unsigned* ws = (unsigned*)workspace;
  OhemRecord* rec = (OhemRecord*)record;
  dim3 grid(pixel_blocks(n, 1024));
  hipLaunchKernelGGL(ohem_zero_kernel, dim3(1), dim3(256), 0, st, ws);                  // kernel node, not memset
  hipLaunchKernelGGL((ohem_hist_kernel<0>), grid, dim3(256), 0, st, q, n, thresh, ws);
  hipLaunchKernelGGL((ohem_scan_kernel<0>), dim3(1), dim3(64), 0, st, ws, min_kept, rec);
  hipLaunchKernelGGL((ohem_hist_kernel<1>), grid, dim3(256), 0, st, q, n, thresh, ws);
  hipLaunchKernelGGL((ohem_scan_kernel<1>), dim3(1), dim3(64), 0, st, ws, min_kept, rec);
  hipLaunchKernelGGL((ohem_hist_kernel<2>), grid, dim3(256), 0, st, q, n, thresh, ws);
  hipLaunchKernelGGL((ohem_scan_kernel<2>), dim3(1), dim3(64), 0, st, ws, min_kept, rec);
  hrseg_count(CNT_OHEM, 7);
  HRSEG_LAUNCH_CHECK("ohem_select");
  return 0;
}
