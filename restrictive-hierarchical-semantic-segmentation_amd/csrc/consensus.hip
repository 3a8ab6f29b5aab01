// Device consensus: M label maps of the same (ragged) images -> one map, voted down the class tree, plus the integer
// counters every inter-map agreement figure follows from.  The semantics are stated in include/hrseg.h under "consensus"
// (hrseg_consensus_labels).  Everything is integer arithmetic, and the counters are sums of integers: the same bytes
// whatever the block order, so there is no deterministic variant.
//
// One launch (family "consensus_labels"), grid (blocks, B) as in score.hip: every sample gets the same number of blocks,
// which stride over the sample's block steps of CONS_BLOCK_STEP pixels; a block past the sample's last step leaves at once.
// The kernel moves M + 1 (+ 1 with support) bytes per pixel; what it has to manage is the counting: up to M L + P L LDS
// updates per pixel.  Real maps are long runs of one member tuple (background on background), so updates are folded twice
// before an LDS atomic is issued:
//   0. setup: thread v reads path_lut[v], drops an entry that is no path (LM_PATH_ENTRY, labelmap_common.h) and keeps it
//      in LDS; the out_val bytes by node and the first node of every level go to LDS as well.
//   1. a lane takes CONS_LANE_STEP = 16 consecutive pixels of all members.  The lane steps are cut at 16-byte boundaries
//      of the OUTPUT span (one aligned 16-byte store); every member's span starts at an unrelated byte, so the lane loads
//      the 5 aligned dwords around its 16 bytes and funnel-shifts them (v_alignbyte), per member.  A member whose aligned
//      window would leave [offset, offset + H*W) of its buffer, and every member of a lane whose 16 pixels are not all
//      inside the image -- only the first and last lanes of an image -- load single bytes instead.  Runs fold in three
//      tiers: all 16 pixels one tuple / a dword of 4 pixels one tuple / single pixels; a tier runs only when some lane of the
//      wave needs it.  The vote and every counter update are made once per folded tuple, with the run's length as count.
//   2. inside a tier every participating lane holds one key per update and the same count (16, 4 or 1): equal keys of a wave
//      are folded before the LDS atomic (lm_wave_add, labelmap_common.h).
//   3. LDS: the cells of hrseg.h, 32-bit (a block counts pixels of ONE image, H*W < 2^31): at most CONS_MAX_CELLS = 2889
//      of them (11.3 KiB) + the 2 KiB path table: a block of 256 lanes, several blocks per CU.
// Flush: every non-zero cell goes to the int64 counters with one 64-bit atomic add.
//
// The vote is byte compares on the packed path entries: at level L member m's byte is compared with every member's; a
// byte that at least `quorum` members share names the level's winner (2 * quorum > M: there is at most one), and the
// deepest winner is the consensus node.  No float arithmetic, no division.
//
// Kept local on purpose: the host check that the M tables agree on every size (cons_host_tables).  It generalises
// lm_host_same_sizes, but its message names members where that one names "predicted map" and "ground truth", and this is
// its only user -- labelmap_common.h holds only what at least two units use.
#include "labelmap_common.h"

#include <cstdio>

#define CONS_TPB 256
#define CONS_LANE_STEP HRSEG_CONSENSUS_LANE_STEP         // 16: the tests take the step sizes from the header
#define CONS_BLOCK_STEP HRSEG_CONSENSUS_BLOCK_STEP
static_assert(CONS_LANE_STEP == 16 && CONS_BLOCK_STEP == CONS_TPB * CONS_LANE_STEP, "hrseg.h states the step sizes of this kernel");
#define CONS_MAX_M HRSEG_CONSENSUS_MAX_MEMBERS
#define CONS_MAX_NODES 64
#define CONS_MAX_PAIRS (CONS_MAX_M * (CONS_MAX_M - 1) / 2)
#define CONS_MAX_CELLS (CONS_MAX_NODES + 1 + 2 * CONS_MAX_NODES * CONS_MAX_M + CONS_MAX_PAIRS * CONS_MAX_NODES + CONS_MAX_M)
static_assert(CONS_MAX_CELLS == 2889, "the cell count hrseg.h states");
#define CONS_BLOCKS 1024                                 // blocks of a launch, over all samples

struct ConsArgs {
  int C[HRSEG_SCORE_MAX_LEVELS];
  int cell0[HRSEG_SCORE_MAX_LEVELS];                     // first node of level L
  unsigned outw[(CONS_MAX_NODES + 4) / 4];               // byte n: out_val of node n; byte `nodes`: none_val
  const u8* buf[CONS_MAX_M];
  int nlevels, nodes, quorum, total, per_image, B;
};

// 16 pixels of M maps: byte j of dword d of member m is pixel 4 d + j; bit 4 d + j of `valid` says the pixel exists
template <int M>
struct ConsTile {
  unsigned t[M][4], valid;
};

template <int M>
__device__ __forceinline__ ConsTile<M> cons_load(const u8* const (&ms)[M], long long i0, long long HW) {
  ConsTile<M> t;
  t.valid = 0;
#pragma unroll
  for (int m = 0; m < M; ++m) {
#pragma unroll
    for (int d = 0; d < 4; ++d) t.t[m][d] = 0;
  }
  if (i0 >= HW || i0 + CONS_LANE_STEP <= 0) return t;
  const bool inside = i0 >= 0 && i0 + CONS_LANE_STEP <= HW;
#pragma unroll
  for (int j = 0; j < CONS_LANE_STEP; ++j)
    if (i0 + j >= 0 && i0 + j < HW) t.valid |= 1u << j;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const uintptr_t ga = (uintptr_t)ms[m] + (uintptr_t)i0, fa = ga & ~(uintptr_t)3;
    if (inside && fa >= (uintptr_t)ms[m] && fa + 20 <= (uintptr_t)ms[m] + (uintptr_t)HW) {
      const unsigned* __restrict__ gw = reinterpret_cast<const unsigned*>(fa);
      const unsigned w0 = gw[0], w1 = gw[1], w2 = gw[2], w3 = gw[3], w4 = gw[4];
      const unsigned sh = (unsigned)(ga & 3);
      t.t[m][0] = __builtin_amdgcn_alignbyte(w1, w0, sh);
      t.t[m][1] = __builtin_amdgcn_alignbyte(w2, w1, sh);
      t.t[m][2] = __builtin_amdgcn_alignbyte(w3, w2, sh);
      t.t[m][3] = __builtin_amdgcn_alignbyte(w4, w3, sh);
    } else {
#pragma unroll
      for (int d = 0; d < 4; ++d) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const long long i = i0 + 4 * d + j;
          if (i >= 0 && i < HW) t.t[m][d] |= (unsigned)ms[m][i] << (8 * j);
        }
      }
    }
  }
  return t;
}

// the layout of a row of counters (hrseg.h): ended, votes, area, both, abstain
struct ConsCells {
  unsigned nodes, votes, area, both, abstain;
};

// one tuple of member bytes v[0..M), `cnt` pixels of it, in every lane with `has`: all counter updates, -> the consensus
// node's output byte and its votes.  Called by whole waves.
template <int M>
__device__ __forceinline__ void cons_tuple(unsigned* cells, const u64* lut, const u8* outv, const int* cell0, const ConsCells k,
                                           int nlevels, unsigned quorum, const unsigned (&v)[M], unsigned cnt, bool has, int lane,
                                           unsigned& out_byte, unsigned& sup_byte) {
  u64 e[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    e[m] = has ? lut[v[m] & 0xffu] : 0ull;
    lm_wave_add(cells, k.abstain + m, cnt, has && e[m] == 0, lane);
  }
  unsigned node = k.nodes, sup = 0;
  for (int L = 0; L < nlevels; ++L) {
    bool left = false;
    unsigned bl[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      left = left || e[m] != 0;
      bl[m] = (unsigned)e[m] & 0xffu;
      e[m] >>= 8;
    }
    if (__ballot(has && left) == 0) break;
    const unsigned c0 = (unsigned)cell0[L];
    int p = 0;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const bool on = has && bl[m] != 0;
      const unsigned n = c0 + bl[m] - 1u;                                  // (only read where `on`)
      lm_wave_add(cells, k.area + m * k.nodes + n, cnt, on, lane);
      unsigned same = 0;
      bool first = true;
#pragma unroll
      for (int o = 0; o < M; ++o) {
        const bool eq = bl[o] == bl[m];
        same += eq ? 1u : 0u;
        if (o < m && eq) first = false;
      }
      lm_wave_add(cells, k.votes + n * M + same - 1u, cnt, on && first, lane);
      if (on && same >= quorum) node = n, sup = same;                     // a deeper winner is a descendant of the last one
#pragma unroll
      for (int o = m + 1; o < M; ++o, ++p) lm_wave_add(cells, k.both + p * k.nodes + n, cnt, on && bl[o] == bl[m], lane);
    }
  }
  lm_wave_add(cells, node, cnt, has, lane);                                // `ended` starts the row
  out_byte = outv[node];
  sup_byte = sup;
}

template <int M>
__global__ __launch_bounds__(CONS_TPB) void consensus_labels_kernel(ConsArgs a, const long long* __restrict__ desc,
                                                                    const u64* __restrict__ path_lut, u8* __restrict__ labels,
                                                                    u8* __restrict__ support, u64* __restrict__ counts) {
  __shared__ unsigned cells[CONS_MAX_CELLS];
  __shared__ u64 lut[256];
  __shared__ unsigned outw[(CONS_MAX_NODES + 4) / 4];
  __shared__ int cell0[HRSEG_SCORE_MAX_LEVELS];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & (HRSEG_WAVE - 1);
  const long long off0 = desc[4 * b], H = desc[4 * b + 1], W = desc[4 * b + 2];
  if (H < 1 || W < 1 || off0 < 0) return;
  if (H > (1ll << 31) / W) return;                                       // H*W > 2^31: the 32-bit block counts could wrap
  const long long HW = H * W;
  const u8* ms[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const long long* row = desc + 4 * ((size_t)m * a.B + b);
    if (row[0] < 0 || row[1] != H || row[2] != W) return;                  // (the host refuses both)
    ms[m] = a.buf[m] + row[0];
  }
  u8* __restrict__ os = labels + off0;                                     // the outputs are packed as member 0 is
  u8* __restrict__ ss = support ? support + off0 : nullptr;
  const int mis = (int)((uintptr_t)os & (CONS_LANE_STEP - 1));              // os - mis is 16-byte aligned
  const long long nsteps = (HW + mis + CONS_BLOCK_STEP - 1) / CONS_BLOCK_STEP;
  if ((long long)blockIdx.x >= nsteps) return;
  const bool sup16 = (((uintptr_t)ss - (uintptr_t)mis) & 15) == 0;

  // ---- setup: zero the counters, the tables to LDS
  for (int i = tid; i < a.total; i += CONS_TPB) cells[i] = 0;
  u64 e = path_lut[tid];                                                 // CONS_TPB == 256: one table entry per thread
  LM_PATH_ENTRY(e, a)
  lut[tid] = e;
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < (CONS_MAX_NODES + 4) / 4; ++i) outw[i] = a.outw[i];
#pragma unroll
    for (int L = 0; L < HRSEG_SCORE_MAX_LEVELS; ++L) cell0[L] = a.cell0[L];
  }
  __syncthreads();
  const u8* outv = reinterpret_cast<const u8*>(outw);
  ConsCells k;
  k.nodes = (unsigned)a.nodes;
  k.votes = k.nodes + 1;
  k.area = k.votes + k.nodes * M;
  k.both = k.area + M * k.nodes;
  k.abstain = k.both + (M * (M - 1) / 2) * k.nodes;
  const int nlevels = a.nlevels;
  const unsigned quorum = (unsigned)a.quorum;

  // ---- vote and count; the next step's loads are in flight while this one is counted
  const long long stride = (long long)gridDim.x * CONS_BLOCK_STEP;
  long long i0 = ((long long)blockIdx.x * CONS_TPB + tid) * CONS_LANE_STEP - mis;
  ConsTile<M> cur = cons_load<M>(ms, i0, HW);
  for (long long s = blockIdx.x; s < nsteps; s += gridDim.x) {
    const ConsTile<M> nxt = cons_load<M>(ms, i0 + stride, HW);           // past the image: an empty tile, nothing is read
    const unsigned valid = cur.valid;
    if (__ballot(valid != 0) != 0) {
      unsigned v[M], ob, sb;
      // tier 1: the 16 pixels are one tuple
      bool one = valid == 0xffffu;
#pragma unroll
      for (int m = 0; m < M; ++m) {
        v[m] = cur.t[m][0] & 0xffu;
        const unsigned splat = v[m] * 0x01010101u;
        one = one && cur.t[m][0] == splat && cur.t[m][1] == splat && cur.t[m][2] == splat && cur.t[m][3] == splat;
      }
      cons_tuple<M>(cells, lut, outv, cell0, k, nlevels, quorum, v, CONS_LANE_STEP, one, lane, ob, sb);
      unsigned o[4], q[4];                                                 // output and support bytes of the 16 pixels
#pragma unroll
      for (int d = 0; d < 4; ++d) o[d] = ob * 0x01010101u, q[d] = sb * 0x01010101u;
      const bool rest = !one && valid != 0;
      if (__ballot(rest) != 0) {
        unsigned vleft = valid;
#pragma unroll 1
        for (int d = 0; d < 4; ++d) {                                      // the dword in turn is always t[m][0]
          const unsigned vd = vleft & 0xfu;
          // tier 2: a dword of 4 pixels is one tuple
          bool four = rest && vd == 0xfu;
#pragma unroll
          for (int m = 0; m < M; ++m) {
            v[m] = cur.t[m][0] & 0xffu;
            four = four && cur.t[m][0] == v[m] * 0x01010101u;
          }
          cons_tuple<M>(cells, lut, outv, cell0, k, nlevels, quorum, v, 4, four, lane, ob, sb);
          unsigned od = four ? ob * 0x01010101u : 0u, qd = four ? sb * 0x01010101u : 0u;
          // tier 3: single pixels
          const bool single = rest && !four && vd != 0;
          if (__ballot(single) != 0) {
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {
              const bool has = single && ((vd >> j) & 1u);
#pragma unroll
              for (int m = 0; m < M; ++m) v[m] = (cur.t[m][0] >> (8 * j)) & 0xffu;
              cons_tuple<M>(cells, lut, outv, cell0, k, nlevels, quorum, v, 1, has, lane, ob, sb);
              if (has) od |= ob << (8 * j), qd |= sb << (8 * j);
            }
          }
          if (rest) {
            o[0] = o[1], o[1] = o[2], o[2] = o[3], o[3] = od;
            q[0] = q[1], q[1] = q[2], q[2] = q[3], q[3] = qd;
          }
#pragma unroll
          for (int m = 0; m < M; ++m) cur.t[m][0] = cur.t[m][1], cur.t[m][1] = cur.t[m][2], cur.t[m][2] = cur.t[m][3];
          vleft >>= 4;
        }
      }
      // ---- store: one aligned 16-byte store where all 16 pixels exist, single bytes at the ragged ends of the image
      if (valid == 0xffffu) {
        u32x4 ov;
        ov[0] = o[0], ov[1] = o[1], ov[2] = o[2], ov[3] = o[3];
        *reinterpret_cast<u32x4*>(os + i0) = ov;
        if (ss) {
          if (sup16) {
            u32x4 qv;
            qv[0] = q[0], qv[1] = q[1], qv[2] = q[2], qv[3] = q[3];
            *reinterpret_cast<u32x4*>(ss + i0) = qv;
          } else {
#pragma unroll
            for (int j = 0; j < CONS_LANE_STEP; ++j) ss[i0 + j] = (u8)(q[j >> 2] >> (8 * (j & 3)));
          }
        }
      } else if (valid != 0) {
#pragma unroll
        for (int j = 0; j < CONS_LANE_STEP; ++j) {
          if ((valid >> j) & 1u) {
            os[i0 + j] = (u8)(o[j >> 2] >> (8 * (j & 3)));
            if (ss) ss[i0 + j] = (u8)(q[j >> 2] >> (8 * (j & 3)));
          }
        }
      }
    }
    i0 += stride;
    cur = nxt;
  }
  __syncthreads();

  // ---- cells -> int64 counters
  const size_t row = a.per_image ? (size_t)b : 0;
  for (int i = tid; i < a.total; i += CONS_TPB)
    if (cells[i]) atomicAdd(&counts[row * a.total + i], (u64)cells[i]);
}

// ------------------------------------------------------------------------------------------------------------ host
// rows [0, B) of the M host tables, each acceptable to lm_host_image (labelmap_common.h), and every member agreeing with
// member 0 on every size
static int cons_host_tables(const char* who, const long* desc_host, int M, int B) {
  for (int m = 0; m < M; ++m) {
    char what[24];
    snprintf(what, sizeof what, "member %d, ", m);
    for (int b = 0; b < B; ++b) {
      long long off, H, W;
      if (int rc = lm_host_image(who, what, desc_host + 4 * (size_t)m * B, b, &off, &H, &W)) return rc;
      const long* first = desc_host + 4 * (size_t)b;
      HRSEG_CHECK_ARG(H == first[1] && W == first[2], "%s: member %d, image %d: %lld x %lld, member 0 has %ld x %ld", who, m, b, H, W,
                      first[1], first[2]);
    }
  }
  return 0;
}

template <int M>
static void cons_launch(const ConsArgs& a, dim3 grid, hipStream_t stream, const long long* desc, const u64* path_lut, u8* labels,
                        u8* support, u64* counts) {
  hipLaunchKernelGGL(consensus_labels_kernel<M>, grid, dim3(CONS_TPB), 0, stream, a, desc, path_lut, labels, support, counts);
}

// ------------------------------------------------------------------------------------------------------------ C ABI
extern "C" int hrseg_consensus_labels(int M, const unsigned char* const* members, const long* desc, const long* desc_host,
                                      const unsigned long long* path_lut, const hrseg_consensus_t* cons, unsigned char* labels,
                                      unsigned char* support, long long* counts, int B, int per_image, hrseg_stream_t stream) {
  const char* who = "hrseg_consensus_labels";
  HRSEG_CHECK_ARG(members && desc && desc_host && path_lut && cons && labels && counts,
                  "%s: null pointer (members, desc, desc_host, path_lut, cons, labels, counts)", who);
  HRSEG_CHECK_ARG(B >= 1 && B <= 65535, "%s: B=%d not in 1..65535", who, B);
  HRSEG_CHECK_ARG(M >= 1 && M <= CONS_MAX_M, "%s: M=%d not in 1..%d", who, M, CONS_MAX_M);
  for (int m = 0; m < M; ++m) HRSEG_CHECK_ARG(members[m], "%s: null pointer (member %d)", who, m);
  HRSEG_CHECK_ARG(2 * (long long)cons->quorum > M && cons->quorum <= M, "%s: quorum %d of %d members: need 2 * quorum > M and quorum <= M",
                  who, cons->quorum, M);
  const int nlevels = cons->nlevels;
  HRSEG_CHECK_ARG(nlevels >= 1 && nlevels <= HRSEG_SCORE_MAX_LEVELS, "%s: nlevels=%d not in 1..%d", who, nlevels, HRSEG_SCORE_MAX_LEVELS);
  ConsArgs a;
  a.nodes = 0;
  for (int L = 0; L < HRSEG_SCORE_MAX_LEVELS; ++L) a.C[L] = a.cell0[L] = 0;
  for (int L = 0; L < nlevels; ++L) {
    HRSEG_CHECK_ARG(cons->C[L] >= 1 && cons->C[L] <= HRSEG_SCORE_MAX_CHANNELS, "%s: C[%d]=%d not in 1..%d", who, L, cons->C[L],
                    HRSEG_SCORE_MAX_CHANNELS);
    a.C[L] = cons->C[L];
    a.cell0[L] = a.nodes;
    a.nodes += cons->C[L];
  }
  HRSEG_CHECK_ARG(a.nodes <= CONS_MAX_NODES, "%s: %d channels over all levels, at most %d", who, a.nodes, CONS_MAX_NODES);
  int owner[256];                                    // 1 + L * 16 + c of the node that writes the byte
  for (int v = 0; v < 256; ++v) owner[v] = 0;
  for (unsigned i = 0; i < sizeof a.outw / sizeof a.outw[0]; ++i) a.outw[i] = 0;
  HRSEG_CHECK_ARG(cons->none_val >= 0 && cons->none_val <= 255, "%s: none_val=%d not in 0..255", who, cons->none_val);
  for (int L = 0; L < nlevels; ++L) {
    for (int c = 0; c < a.C[L]; ++c) {
      const int v = cons->out_val[L][c], n = a.cell0[L] + c;
      HRSEG_CHECK_ARG(v >= 0 && v <= 255, "%s: (level %d, channel %d) has the output value %d, not in 0..255", who, L, c, v);
      HRSEG_CHECK_ARG(v != cons->none_val, "%s: (level %d, channel %d) and none_val share the byte %d", who, L, c, v);
      HRSEG_CHECK_ARG(owner[v] == 0, "%s: (level %d, channel %d) and (level %d, channel %d) share the byte %d", who,
                      (owner[v] - 1) / HRSEG_SCORE_MAX_CHANNELS, (owner[v] - 1) % HRSEG_SCORE_MAX_CHANNELS, L, c, v);
      owner[v] = 1 + L * HRSEG_SCORE_MAX_CHANNELS + c;
      a.outw[n >> 2] |= (unsigned)v << (8 * (n & 3));
    }
  }
  a.outw[a.nodes >> 2] |= (unsigned)cons->none_val << (8 * (a.nodes & 3));
  if (int rc = cons_host_tables(who, desc_host, M, B)) return rc;
  HRSEG_CHECK_ARG(((uintptr_t)counts & 7) == 0 && ((uintptr_t)path_lut & 7) == 0, "%s: counts and path_lut must be 8-byte aligned", who);
  HRSEG_CHECK_ARG(((uintptr_t)labels & 3) == 0, "%s: labels must be 4-byte aligned", who);
  for (int m = 0; m < CONS_MAX_M; ++m) a.buf[m] = m < M ? members[m] : nullptr;
  a.nlevels = nlevels;
  a.quorum = cons->quorum;
  a.total = a.nodes + 1 + 2 * a.nodes * M + (M * (M - 1) / 2) * a.nodes + M;
  a.per_image = per_image ? 1 : 0;
  a.B = B;
  int per_sample = (CONS_BLOCKS + B - 1) / B;
  per_sample = per_sample < 1 ? 1 : per_sample;
  const dim3 grid((unsigned)per_sample, (unsigned)B);
  const long long* d = (const long long*)desc;
  const u64* lut = (const u64*)path_lut;
  u64* cnt = (u64*)counts;
  hipStream_t st = (hipStream_t)stream;
  switch (M) {
    case 1: cons_launch<1>(a, grid, st, d, lut, labels, support, cnt); break;
    case 2: cons_launch<2>(a, grid, st, d, lut, labels, support, cnt); break;
    case 3: cons_launch<3>(a, grid, st, d, lut, labels, support, cnt); break;
    case 4: cons_launch<4>(a, grid, st, d, lut, labels, support, cnt); break;
    case 5: cons_launch<5>(a, grid, st, d, lut, labels, support, cnt); break;
    case 6: cons_launch<6>(a, grid, st, d, lut, labels, support, cnt); break;
    case 7: cons_launch<7>(a, grid, st, d, lut, labels, support, cnt); break;
    default: cons_launch<8>(a, grid, st, d, lut, labels, support, cnt); break;
  }
  HRSEG_LAUNCH_CHECK("consensus_labels");
  hrseg_count(CNT_CONSENSUS_LABELS);
  return 0;
}
