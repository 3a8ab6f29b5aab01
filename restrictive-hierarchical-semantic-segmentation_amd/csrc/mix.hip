// Mixing augmentation across the samples of a batch (ClassMix / CutMix / paste by tree node): per-channel pixel counts, the
// paste mask with its node choice, and the masked gather.  The semantics are stated once, in include/hrseg.h ("mixing");
// Data/mix.py draws the per-sample table.  All three kernels are HBM-bound passes over [B,*,S,S] planes.  gfx950.
//
// Planes start wherever (b*K + k)*S*S puts them, so with S*S % 4 != 0 they leave the 16-byte grid.  Every kernel therefore
// walks a plane in a SHIFTED index j = i + a, a = the plane start's offset in elements from the 16-byte grid of what the
// kernel stores (or, for the counts, loads): a group j..j+3 with j % 4 == 0 is aligned, groups that straddle the plane's ends
// take the scalar path.  The other side of a group (the donor, moved by dx + dy*S elements, and the 4 mask bytes of the
// gather) is read through 4-byte- resp. 1-byte-aligned vector types: one wide load wherever it happens to sit.
#include "common.h"

typedef unsigned u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));   // 16 bytes at any element boundary
typedef unsigned u32_a1 __attribute__((aligned(1)));                         // 4 mask bytes at any byte

#define MIX_THREADS 256
#define MIX_GROUP 4                                      // consecutive pixels per thread
#define MIX_CHUNK (MIX_THREADS * MIX_GROUP)              // shifted indices per block of the masks kernel, per round of the others
#define MIX_COUNT_VECS 4                                 // 16-byte groups per thread of the counts kernel
#define MIX_COUNT_CHUNK (MIX_CHUNK * MIX_COUNT_VECS)

static inline long mix_chunks(long hw, long chunk) { return (hw + 3 + chunk - 1) / chunk; }   // covers any shift a <= 3
// `planes` planes of S x S elements stay below 2^31 elements (without forming a product that could overflow)
static inline bool mix_fits(long planes, int S) {
  const long hw = (long)S * S;
  return hw < (1l << 31) && planes <= ((1l << 31) - 1) / hw;
}

#define ONE_BITS 0x3f800000u                             // y == 1.0f has exactly these bits

// --------------------------------------------------------------------------- counts
// counts[b][c] += |{y[b][c] == 1.0f}| over the block's share of one plane: 16-byte loads (all of a round issued before the first
// is looked at), wave sum, 4 wave sums through LDS, one integer atomic per block (none where the share holds no 1).  A plane is
// dealt to at most MIX_COUNT_BLOCKS blocks, chunk by chunk: the atomics on one address queue up behind each other, and with
// one block per chunk (94 per plane at 620 x 620) that queue, not the loads, set the kernel's time.
#define MIX_COUNT_BLOCKS 16
__global__ __launch_bounds__(MIX_THREADS) void mix_counts_kernel(const unsigned* __restrict__ y, int* __restrict__ counts, long hw,
                                                                 int chunks, int per_plane) {
  __shared__ int part[MIX_THREADS / HRSEG_WAVE];
  const long plane = blockIdx.x / per_plane;
  const int share = blockIdx.x - (int)(plane * per_plane);
  const unsigned* p = y + plane * hw;
  const long a = (long)(((uintptr_t)p >> 2) & 3);
  int n = 0;
  for (int chunk = share; chunk < chunks; chunk += per_plane) {
    long idx[MIX_COUNT_VECS];
    u32x4 q[MIX_COUNT_VECS];
#pragma unroll
    for (int v = 0; v < MIX_COUNT_VECS; ++v) {
      idx[v] = (long)chunk * MIX_COUNT_CHUNK + ((long)v * MIX_THREADS + threadIdx.x) * MIX_GROUP - a;
      q[v] = u32x4{0u, 0u, 0u, 0u};
      if (idx[v] >= 0 && idx[v] + MIX_GROUP <= hw) q[v] = *reinterpret_cast<const u32x4*>(p + idx[v]);
    }
#pragma unroll
    for (int v = 0; v < MIX_COUNT_VECS; ++v) {
      n += (q[v][0] == ONE_BITS) + (q[v][1] == ONE_BITS) + (q[v][2] == ONE_BITS) + (q[v][3] == ONE_BITS);
      if (!(idx[v] >= 0 && idx[v] + MIX_GROUP <= hw)) {     // a group across the plane's start or end: element by element
#pragma unroll
        for (int e = 0; e < MIX_GROUP; ++e)
          if (idx[v] + e >= 0 && idx[v] + e < hw) n += p[idx[v] + e] == ONE_BITS;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < MIX_THREADS / HRSEG_WAVE; ++w) s += part[w];
    if (s) atomicAdd(counts + plane, s);
  }
}

extern "C" int hrseg_mix_counts(const float* y, int* counts, int B, int C, long hw, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(y && counts, "hrseg_mix_counts: null pointer");
  HRSEG_CHECK_ARG(B >= 1, "hrseg_mix_counts: B=%d below 1", B);
  HRSEG_CHECK_ARG(C >= 1 && C <= 64, "hrseg_mix_counts: C=%d not in 1..64", C);
  HRSEG_CHECK_ARG(hw >= 1 && hw < (1l << 31), "hrseg_mix_counts: hw=%ld not in 1..2^31-1", hw);
  const long chunks = mix_chunks(hw, MIX_COUNT_CHUNK), per_plane = chunks < MIX_COUNT_BLOCKS ? chunks : MIX_COUNT_BLOCKS;
  const long blocks = per_plane * B * C;                  // (below 2^31 * 64 * 16: no overflow)
  HRSEG_CHECK_ARG(blocks < (1l << 31), "hrseg_mix_counts: B=%d samples are more than one launch holds", B);
  if (hipMemsetAsync(counts, 0, sizeof(int) * (size_t)B * C, (hipStream_t)stream) != hipSuccess) {
    hrseg_set_error("hrseg_mix_counts: clearing the counts failed");
    return HRSEG_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(mix_counts_kernel, dim3((unsigned)blocks), dim3(MIX_THREADS), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned*>(y), counts, hw, (int)chunks, (int)per_plane);
  HRSEG_LAUNCH_CHECK("hrseg_mix_counts");
  hrseg_count(CNT_MIX);
  return 0;
}

// --------------------------------------------------------------------------- what masks and gather share
// One sample's row of the table, read by every thread of a block from the same address.  A donor outside [0,B) switches the
// sample off: the table is device memory that the host validated, and no kernel here indexes with a value it has not checked.
struct MixSample { bool apply, box; int donor, dx, dy, r0, c0, r1, c1; };
__device__ __forceinline__ MixSample mix_sample(const int* __restrict__ params, int b, int B) {
  const int* p = params + (size_t)b * HRSEG_MIX_PARAMS;
  MixSample s;
  const int flags = p[HRSEG_MIX_P_FLAGS];
  s.donor = p[HRSEG_MIX_P_DONOR];
  s.apply = (flags & HRSEG_MIX_APPLY) && s.donor >= 0 && s.donor < B;
  s.box = flags & HRSEG_MIX_BOX;
  s.dx = p[HRSEG_MIX_P_DX], s.dy = p[HRSEG_MIX_P_DY];
  s.r0 = p[HRSEG_MIX_P_BOX], s.c0 = p[HRSEG_MIX_P_BOX + 1], s.r1 = p[HRSEG_MIX_P_BOX + 2], s.c1 = p[HRSEG_MIX_P_BOX + 3];
  return s;
}

// bit e: pixel i + e of the plane exists and its donor pixel (r - dy, c - dx) lies in the frame; also the pixel's row and column
struct MixGroup { unsigned inframe; int r[MIX_GROUP], c[MIX_GROUP]; };
__device__ __forceinline__ MixGroup mix_group(long i, int S, long hw, const MixSample& s) {
  MixGroup g;
  g.inframe = 0;
  const unsigned i0 = i < 0 ? 0u : (unsigned)i;          // (hw < 2^31: a 32-bit division)
  int r = (int)(i0 / (unsigned)S), c = (int)(i0 - (unsigned)r * (unsigned)S);
#pragma unroll
  for (int e = 0; e < MIX_GROUP; ++e) {
    g.r[e] = r, g.c[e] = c;
    if (i + e >= 0 && i + e < hw) {
      const long sr = (long)r - s.dy, sc = (long)c - s.dx;
      if (sr >= 0 && sr < S && sc >= 0 && sc < S) g.inframe |= 1u << e;
      if (++c == S) c = 0, ++r;
    }
  }
  return g;
}

// --------------------------------------------------------------------------- masks
// Block (sample b, chunk): wave 0 rebuilds chosen[b] (at most 64 candidates: a ballot for n, a rank by counting smaller
// priorities), then every thread writes 4 mask bytes from the chosen channels of the donor alone.
__global__ __launch_bounds__(MIX_THREADS) void mix_masks_kernel(const unsigned* __restrict__ y, const int* __restrict__ counts,
                                                                const int* __restrict__ params, const int* __restrict__ prio,
                                                                const int* __restrict__ k_of_n, unsigned long long cand,
                                                                int min_pixels, unsigned char* __restrict__ mask,
                                                                unsigned long long* __restrict__ chosen_out, int B, int C, int S,
                                                                int chunks) {
  __shared__ int s_prio[HRSEG_WAVE];
  __shared__ unsigned long long s_chosen;
  const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
  const MixSample s = mix_sample(params, b, B);
  const long hw = (long)S * S;
  const bool pick = s.apply && !s.box;                  // (uniform over the block)
  if (pick) {
    const int t = threadIdx.x;
    bool present = false;
    int pr = 0x7fffffff;
    if (t < HRSEG_WAVE) {
      present = counts && t < C && ((cand >> t) & 1) && counts[(size_t)s.donor * C + t] >= min_pixels;
      if (present) pr = prio[(size_t)b * C + t];
      s_prio[t] = pr;
    }
    __syncthreads();
    if (t < HRSEG_WAVE) {
      const unsigned long long have = __ballot(present);
      const int k = k_of_n[__popcll(have)];
      int rank = 0;
      for (int j = 0; j < C; ++j) {
        const int pj = s_prio[j];
        rank += ((have >> j) & 1) && (pj < pr || (pj == pr && j < t));
      }
      const unsigned long long chosen = __ballot(present && rank < k);
      if (t == 0) s_chosen = chosen;
    }
    __syncthreads();
  }
  const unsigned long long chosen = pick ? s_chosen : 0ull;
  if (chunk == 0 && threadIdx.x == 0) chosen_out[b] = chosen;

  unsigned char* m = mask + (size_t)b * hw;
  const long a = (long)((uintptr_t)m & 3);
  const long i = (long)chunk * MIX_CHUNK + (long)threadIdx.x * MIX_GROUP - a;
  if (i + MIX_GROUP <= 0 || i >= hw) return;
  unsigned hit = 0;                                      // bit e: pixel i + e is pasted
  if (s.apply) {
    const MixGroup g = mix_group(i, S, hw, s);
    if (s.box) {
#pragma unroll
      for (int e = 0; e < MIX_GROUP; ++e)
        if (g.r[e] >= s.r0 && g.r[e] < s.r1 && g.c[e] >= s.c0 && g.c[e] < s.c1) hit |= 1u << e;
      hit &= g.inframe;
    } else if (g.inframe) {
      const long off = (long)s.dy * S + s.dx;            // an in-frame donor pixel sits at flat index i + e - off
      unsigned long long rest = chosen;
      while (rest && hit != g.inframe) {
        const int c = __ffsll((long long)rest) - 1;
        rest &= rest - 1;
        const unsigned* p = y + ((size_t)s.donor * C + c) * hw;
        if (g.inframe == 0xfu) {
          const u32x4_a4 q = *reinterpret_cast<const u32x4_a4*>(p + (i - off));
#pragma unroll
          for (int e = 0; e < MIX_GROUP; ++e) hit |= (unsigned)(q[e] == ONE_BITS) << e;
        } else {
#pragma unroll
          for (int e = 0; e < MIX_GROUP; ++e)
            if (((g.inframe >> e) & 1) && p[i + e - off] == ONE_BITS) hit |= 1u << e;
        }
      }
    }
  }
  if (i >= 0 && i + MIX_GROUP <= hw) {
    *reinterpret_cast<unsigned*>(m + i) = (hit & 1) | ((hit & 2) << 7) | ((hit & 4) << 14) | ((hit & 8) << 21);
  } else {
#pragma unroll
    for (int e = 0; e < MIX_GROUP; ++e)
      if (i + e >= 0 && i + e < hw) m[i + e] = (hit >> e) & 1;
  }
}

extern "C" int hrseg_mix_masks(const float* y, const int* counts, const int* params, const int* prio, const int* k_of_n,
                               const int* cand, int min_pixels, unsigned char* mask, unsigned long long* chosen, int B, int C,
                               int S, hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(y && params && prio && k_of_n && cand && mask && chosen, "hrseg_mix_masks: null pointer");
  HRSEG_CHECK_ARG(B >= 1, "hrseg_mix_masks: B=%d below 1", B);
  HRSEG_CHECK_ARG(C >= 1 && C <= 64, "hrseg_mix_masks: C=%d not in 1..64", C);
  HRSEG_CHECK_ARG(S >= 1, "hrseg_mix_masks: S=%d below 1", S);
  HRSEG_CHECK_ARG(mix_fits((long)B * C, S), "hrseg_mix_masks: B*C*S*S=%d*%d*%d*%d is 2^31 or more", B, C, S, S);
  HRSEG_CHECK_ARG(min_pixels >= 1, "hrseg_mix_masks: min_pixels=%d below 1", min_pixels);
  unsigned long long bits = 0;
  for (int c = 0; c < C; ++c) bits |= (unsigned long long)(cand[c] != 0) << c;
  const long chunks = mix_chunks((long)S * S, MIX_CHUNK);
  hipLaunchKernelGGL(mix_masks_kernel, dim3((unsigned)(chunks * B)), dim3(MIX_THREADS), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned*>(y), counts, params, prio, k_of_n, bits, min_pixels, mask, chosen, B, C, S,
                     (int)chunks);
  HRSEG_LAUNCH_CHECK("hrseg_mix_masks");
  hrseg_count(CNT_MIX);
  return 0;
}

// --------------------------------------------------------------------------- gather
// Block (plane b*K + k, chunk); a thread moves MIX_GATHER_VECS groups of 4 consecutive elements as bits: the recipient's where
// none is pasted (one 16-byte load), the donor's where all four are (one 16-byte load at the moved address), the recipient's
// patched element by element on the seams.  The thread issues its mask loads, then its data loads, then stores, so that several
// loads are in flight per lane.  A set mask byte is honoured only where the sample is applied and the donor pixel lies in the
// frame, so no mask can make the kernel read outside `in`.
#define MIX_GATHER_VECS 4
#define MIX_GATHER_CHUNK (MIX_CHUNK * MIX_GATHER_VECS)
__global__ __launch_bounds__(MIX_THREADS) void mix_gather_kernel(const unsigned* __restrict__ in, const unsigned char* __restrict__ mask,
                                                                 const int* __restrict__ params, unsigned* __restrict__ out, int B,
                                                                 int K, int S, int chunks) {
  const int plane = blockIdx.x / chunks, chunk = blockIdx.x - plane * chunks;
  const int b = plane / K, k = plane - b * K;
  const MixSample s = mix_sample(params, b, B);
  const long hw = (long)S * S;
  unsigned* o = out + (size_t)plane * hw;
  const unsigned* mine = in + (size_t)plane * hw;
  const unsigned char* m = mask + (size_t)b * hw;
  const long a = (long)(((uintptr_t)o >> 2) & 3);
  // element i of the donor's moved plane is in[theirs + i] (formed for every group, read only where `take` says so)
  const long theirs = ((long)(s.apply ? s.donor : b) * K + k) * hw - ((long)s.dy * S + s.dx);
  const long first = (long)chunk * MIX_GATHER_CHUNK + (long)threadIdx.x * MIX_GROUP - a;   // group u starts at first + u * MIX_CHUNK
  unsigned w[MIX_GATHER_VECS], take[MIX_GATHER_VECS];      // take, bit e: element i + e comes from the donor
  u32x4 v[MIX_GATHER_VECS];
  // The loads of a phase stand in straight-line code: a group that is not whole reads the plane's first or last whole group
  // instead (and drops it), so that no branch keeps one load from being issued behind the other.
  if (hw >= MIX_GROUP) {
#pragma unroll
    for (int u = 0; u < MIX_GATHER_VECS; ++u) take[u] = 0;
    if (s.apply) {
#pragma unroll
      for (int u = 0; u < MIX_GATHER_VECS; ++u) {
        const long i = first + (long)u * MIX_CHUNK;
        w[u] = *reinterpret_cast<const u32_a1*>(m + min(max(i, 0l), hw - MIX_GROUP));
      }
#pragma unroll
      for (int u = 0; u < MIX_GATHER_VECS; ++u) {
        const long i = first + (long)u * MIX_CHUNK;
        if (w[u] && i >= 0 && i + MIX_GROUP <= hw) {
          take[u] = ((w[u] & 0xffu) != 0) | (((w[u] & 0xff00u) != 0) << 1) | (((w[u] & 0xff0000u) != 0) << 2) | (((w[u] >> 24) != 0) << 3);
          take[u] &= mix_group(i, S, hw, s).inframe;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < MIX_GATHER_VECS; ++u) {
      const long i = first + (long)u * MIX_CHUNK;
      const long from = take[u] == 0xfu ? theirs + i : (long)plane * hw + min(max(i, 0l), hw - MIX_GROUP);
      v[u] = *reinterpret_cast<const u32x4_a4*>(in + from);
    }
#pragma unroll
    for (int u = 0; u < MIX_GATHER_VECS; ++u) {
      const long i = first + (long)u * MIX_CHUNK;
      if (i >= 0 && i + MIX_GROUP <= hw) {
        if (take[u] != 0 && take[u] != 0xfu) {
#pragma unroll
          for (int e = 0; e < MIX_GROUP; ++e)
            if ((take[u] >> e) & 1) v[u][e] = in[theirs + i + e];
        }
        *reinterpret_cast<u32x4*>(o + i) = v[u];
      }
    }
  }
  // a group across the plane's start or end (at most two per plane): element by element
#pragma nounroll
  for (int u = 0; u < MIX_GATHER_VECS; ++u) {
    const long i = first + (long)u * MIX_CHUNK;
    if ((i >= 0 && i + MIX_GROUP <= hw) || i + MIX_GROUP <= 0 || i >= hw) continue;
    unsigned t = 0;
    if (s.apply) {
#pragma unroll
      for (int e = 0; e < MIX_GROUP; ++e)
        if (i + e >= 0 && i + e < hw && m[i + e]) t |= 1u << e;
      if (t) t &= mix_group(i, S, hw, s).inframe;
    }
#pragma unroll
    for (int e = 0; e < MIX_GROUP; ++e)
      if (i + e >= 0 && i + e < hw) o[i + e] = ((t >> e) & 1) ? in[theirs + i + e] : mine[i + e];
  }
}

extern "C" int hrseg_mix_gather(const float* in, const unsigned char* mask, const int* params, float* out, int B, int K, int S,
                                hrseg_stream_t stream) {
  HRSEG_CHECK_ARG(in && mask && params && out, "hrseg_mix_gather: null pointer");
  HRSEG_CHECK_ARG(B >= 1, "hrseg_mix_gather: B=%d below 1", B);
  HRSEG_CHECK_ARG(K >= 1, "hrseg_mix_gather: K=%d below 1", K);
  HRSEG_CHECK_ARG(S >= 1, "hrseg_mix_gather: S=%d below 1", S);
  HRSEG_CHECK_ARG(mix_fits((long)B * K, S), "hrseg_mix_gather: B*K*S*S=%d*%d*%d*%d is 2^31 or more", B, K, S, S);
  HRSEG_CHECK_ARG(in != out, "hrseg_mix_gather: out must not alias in (a donor can itself be a recipient)");
  const long chunks = mix_chunks((long)S * S, MIX_GATHER_CHUNK);
  hipLaunchKernelGGL(mix_gather_kernel, dim3((unsigned)(chunks * B * K)), dim3(MIX_THREADS), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned*>(in), mask, params, reinterpret_cast<unsigned*>(out), B, K, S, (int)chunks);
  HRSEG_LAUNCH_CHECK("hrseg_mix_gather");
  hrseg_count(CNT_MIX);
  return 0;
}
