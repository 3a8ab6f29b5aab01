// Device instance scoring: the connected components of a predicted and a ground-truth label map are matched one to one
// (IoU > 1/2) and counted per group of the cut and image.  The semantics are stated in include/hrseg.h
// (hrseg_mask_void_labels, hrseg_score_instances); everything is integer arithmetic and every output is decided by exact
// tests on integers: the same bytes whatever order the blocks and atomics run in.
//
// No pair table: the (P, G) pairs of two maps are bounded by the pixel count only.  A partner of G holds more than half of
// G's pixels (3 inter > |P| + |G| and |P| >= inter give 2 inter > |G|), so a Boyer-Moore majority vote over G's pixels finds
// the one component that can be it, one 64-bit slot per true component; the overlap with that candidate alone is counted
// and the exact test decides.  Where no partner exists the vote ends on some run-dependent candidate, which then fails the
// test like every other one would: the intermediate state depends on the run, the outputs do not.
//
// No block waits for another one; kernel boundaries do the ordering.
// hrseg_mask_void_labels, 1 launch: in_mask_kernel copies the prediction, void_value where the ground truth has group 255.
// hrseg_score_instances, 4 launches (all counted under the family "score_instances"), grid (steps of the largest image, B):
//   1. in_init_kernel zeroes the slot and the overlap of every ground-truth pixel, writes pmatch (-1 at the first pixel of a
//      predicted thing component, -2 elsewhere) and counts n_gt / n_pred per block in LDS, one 64-bit add per non-zero cell.
//   2. in_walk_kernel<false>, the vote: a wave walks IN_CHUNK consecutive pixels, 64 at a time.  A lane's key is (g_root,
//      p_root or "none"); a run of equal keys inside the 64 is found by a ballot and leaves as ONE weighted vote from its
//      first lane; the run that touches the end of the 64 is carried into the next 64, so the inside of a large component
//      costs one compare-and-swap per IN_CHUNK pixels.  Pixels of groups that are no things do not vote.
//   3. in_walk_kernel<true>, the count: the same runs; where p_root is the slot's candidate the run adds its length to
//      inter[g_root].
//   4. in_decide_kernel: at every true first pixel of a thing group the test 3 inter > |P| + |G| with the candidate's area;
//      gmatch, ginter and pmatch[candidate] are written (a P has at most one partner: no two writers), the sums per block
//      in LDS, then one 64-bit add per non-zero cell.
#include "labelmap_common.h"

#define IN_TPB 256
#define IN_WAVES (IN_TPB / HRSEG_WAVE)
#define IN_STEPS 16                                    // pixels per thread of the mask / init / decide kernels
#define IN_CHUNK 2048                                  // consecutive pixels a wave of the vote / count kernels walks
#define IN_NONE 0xffffffffu                            // the vote of a pixel without a predicted component of G's group
#define IN_FIELDS HRSEG_INSTANCE_FIELDS
#define IN_SUMS (IN_FIELDS - 2)                        // the fields the decide kernel adds: tp .. tp_at[3]
static_assert(IN_TPB == 256, "one thread per entry of the group tables");
static_assert(IN_FIELDS == 10 && IN_CHUNK % HRSEG_WAVE == 0, "hrseg.h states the record's fields");

struct InImage {
  long long poff, goff, HW;
  bool ok;
};

// image b of both tables.  Not ok -- skipped by every launch -- when a DEVICE descriptor breaks a rule the host table was
// checked for, when the two tables disagree on the size, or when a span would leave the extent the host computed (and
// sized the workspace by): no index below ever leaves [0, extent) of its buffer.
__device__ __forceinline__ InImage in_image(const long long* __restrict__ pdesc, const long long* __restrict__ gdesc, int b, long long pext,
                                            long long gext) {
  InImage im;
  const long long H = pdesc[4 * b + 1], W = pdesc[4 * b + 2];
  im.poff = pdesc[4 * b];
  im.goff = gdesc[4 * b];
  im.ok = H >= 1 && W >= 1 && im.poff >= 0 && im.goff >= 0 && H <= ((1ll << 31) - 1) / W && gdesc[4 * b + 1] == H && gdesc[4 * b + 2] == W;
  im.HW = im.ok ? H * W : 0;
  im.ok = im.ok && im.poff + im.HW <= pext && im.goff + im.HW <= gext;
  return im;
}

// ------------------------------------------------------------------------------------------------ the masked copy
__global__ __launch_bounds__(IN_TPB) void in_mask_kernel(const u8* __restrict__ pred, const long long* __restrict__ pdesc,
                                                         const u8* __restrict__ gt, const long long* __restrict__ gdesc,
                                                         const u8* __restrict__ group, int void_value, u8* __restrict__ out, long long pext,
                                                         long long gext) {
  __shared__ u8 lut[256];
  const int tid = threadIdx.x;
  lut[tid] = group[tid];
  __syncthreads();
  const InImage im = in_image(pdesc, gdesc, blockIdx.y, pext, gext);
  if (!im.ok) return;
  const long long base = (long long)blockIdx.x * (IN_TPB * IN_STEPS);
  for (int k = 0; k < IN_STEPS; ++k) {
    const long long i = base + (long long)k * IN_TPB + tid;
    if (i >= im.HW) break;
    u8 v = pred[im.poff + i];
    if (void_value >= 0 && lut[gt[im.goff + i]] == 255) v = (u8)void_value;
    out[im.poff + i] = v;
  }
}

// ------------------------------------------------------------------------------------------------ 1. clear and count
__global__ __launch_bounds__(IN_TPB) void in_init_kernel(const u8* __restrict__ pm, const long long* __restrict__ pdesc,
                                                         const u8* __restrict__ gt, const long long* __restrict__ gdesc,
                                                         const u8* __restrict__ group, const u8* __restrict__ things,
                                                         const int* __restrict__ parea, const int* __restrict__ garea, u64* __restrict__ slot,
                                                         u32* __restrict__ inter, int* __restrict__ pmatch, u64* __restrict__ records,
                                                         int per_image, long long pext, long long gext) {
  __shared__ u8 lut[256], th[256];
  __shared__ u32 hist[2 * 256];                                                // n_gt, n_pred of this block per group
  const int tid = threadIdx.x, b = blockIdx.y;
  lut[tid] = group[tid];
  th[tid] = tid != 255 && things[tid] != 0;
  hist[tid] = hist[256 + tid] = 0;
  __syncthreads();
  const InImage im = in_image(pdesc, gdesc, b, pext, gext);
  if (!im.ok) return;
  const long long base = (long long)blockIdx.x * (IN_TPB * IN_STEPS);
  if (base >= im.HW) return;
  for (int k = 0; k < IN_STEPS; ++k) {
    const long long i = base + (long long)k * IN_TPB + tid;
    if (i >= im.HW) break;
    const long long gi = im.goff + i, pi = im.poff + i;
    slot[gi] = 0;
    inter[gi] = 0;
    if (garea[gi] > 0) {
      const int g = lut[gt[gi]];
      if (th[g]) atomicAdd(&hist[g], 1u);
    }
    int m = -2;
    if (parea[pi] > 0) {
      const int g = lut[pm[pi]];
      if (th[g]) {
        atomicAdd(&hist[256 + g], 1u);
        m = -1;
      }
    }
    pmatch[pi] = m;
  }
  __syncthreads();
  u64* rec = records + (size_t)(per_image ? b : 0) * 256 * IN_FIELDS + (size_t)tid * IN_FIELDS;
  if (hist[tid]) atomicAdd(&rec[0], (u64)hist[tid]);
  if (hist[256 + tid]) atomicAdd(&rec[1], (u64)hist[256 + tid]);
}

// ------------------------------------------------------------------------------------------------ 2. vote, 3. count
// one weighted Boyer-Moore vote (key, w >= 1) into the slot (candidate << 32 | count); count 0 is the empty slot.  It equals
// w unit votes in sequence: an empty slot takes the vote, the candidate's own vote adds, another's subtracts, and what is
// left of the vote behind count 0 takes the slot over.  The votes of one component sum to its area < 2^31.
// Bounded: lock-free -- a compare-and-swap fails only because another vote landed, and every vote lands once.
__device__ __forceinline__ void in_vote(u64* p, u32 key, u32 w) {
  u64 old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (;;) {
    const u32 c = (u32)(old >> 32), n = (u32)old;
    u64 nw;
    if (n == 0)
      nw = ((u64)key << 32) | w;
    else if (c == key)
      nw = old + w;
    else if (n >= w)
      nw = ((u64)c << 32) | (n - w);
    else
      nw = ((u64)key << 32) | (w - n);
    const u64 seen = atomicCAS(p, old, nw);
    if (seen == old) return;
    old = seen;
  }
}

// the candidate of a slot the vote left behind (IN_NONE: there is none, or it is "no component")
__device__ __forceinline__ u32 in_candidate(u64 s) { return (u32)s != 0 ? (u32)(s >> 32) : IN_NONE; }

template <bool COUNT>
__device__ __forceinline__ void in_emit(u64* S, u32* I, int g, u32 key, u32 n) {
  if (COUNT) {
    if (key != IN_NONE && in_candidate(S[g]) == key) atomicAdd(&I[g], n);
  } else {
    in_vote(&S[g], key, n);
  }
}

template <bool COUNT>
__global__ __launch_bounds__(IN_TPB) void in_walk_kernel(const u8* __restrict__ pm, const long long* __restrict__ pdesc,
                                                         const u8* __restrict__ gt, const long long* __restrict__ gdesc,
                                                         const u8* __restrict__ group, const u8* __restrict__ things,
                                                         const int* __restrict__ proots, const int* __restrict__ groots, u64* __restrict__ slot,
                                                         u32* __restrict__ inter, long long pext, long long gext) {
  __shared__ u8 lut[256], th[256];
  const int tid = threadIdx.x, wave = tid / HRSEG_WAVE, lane = tid & (HRSEG_WAVE - 1);
  lut[tid] = group[tid];
  th[tid] = tid != 255 && things[tid] != 0;
  __syncthreads();
  const InImage im = in_image(pdesc, gdesc, blockIdx.y, pext, gext);
  if (!im.ok) return;
  const long long base = ((long long)blockIdx.x * IN_WAVES + wave) * IN_CHUNK;
  if (base >= im.HW) return;                                                  // (whole waves leave; no barrier follows)
  const u8* __restrict__ P = pm + im.poff;
  const u8* __restrict__ G = gt + im.goff;
  const int* __restrict__ PR = proots + im.poff;
  const int* __restrict__ GR = groots + im.goff;
  u64* S = slot + im.goff;
  u32* I = inter + im.goff;
  // the run that touched the end of the last 64 pixels: the same values in every lane (pn == 0: none)
  int pg = -1;
  u32 pk = IN_NONE, pn = 0;
  for (int it = 0; it < IN_CHUNK / HRSEG_WAVE; ++it) {
    const long long i0 = base + (long long)it * HRSEG_WAVE, i = i0 + lane;
    if (i0 >= im.HW) break;
    // the key: g < 0 = this pixel does not vote (outside the image, or its true component is no thing)
    int g = -1;
    u32 k = IN_NONE;
    if (i < im.HW) {
      const int gg = lut[G[i]];
      if (th[gg]) {
        const int r = GR[i];
        if (r >= 0 && r < im.HW) {                                             // (always, for roots hrseg_label_components wrote)
          g = r;
          if (lut[P[i]] == gg) k = (u32)PR[i];
        }
      }
    }
    const int gl = __shfl_up(g, 1, HRSEG_WAVE);
    const u32 kl = __shfl_up(k, 1, HRSEG_WAVE);
    const bool head = lane == 0 || g != gl || k != kl;
    const u64 heads = __ballot(head);                                         // bit 0 is always set
    const u64 above = lane == HRSEG_WAVE - 1 ? 0ull : heads >> (lane + 1);
    u32 n = above ? (u32)__ffsll((long long)above) : (u32)(HRSEG_WAVE - lane);  // pixels up to the next head
    const int last = 63 - __clzll((long long)heads);                          // the head of the run that touches the end
    // the carried run goes on in lane 0's run, or leaves
    if (pn) {
      const int g0 = __shfl(g, 0, HRSEG_WAVE);
      const u32 k0 = __shfl(k, 0, HRSEG_WAVE);
      if (g0 == pg && k0 == pk) {
        if (lane == 0) n += pn;
      } else if (lane == 0) {
        in_emit<COUNT>(S, I, pg, pk, pn);
      }
      pn = 0;
    }
    pg = __shfl(g, last, HRSEG_WAVE);
    pk = __shfl(k, last, HRSEG_WAVE);
    pn = pg >= 0 ? __shfl(n, last, HRSEG_WAVE) : 0u;
    if (head && lane != last && g >= 0) in_emit<COUNT>(S, I, g, k, n);
  }
  if (pn && lane == 0) in_emit<COUNT>(S, I, pg, pk, pn);
}

// ------------------------------------------------------------------------------------------------ 4. decide
struct InThresholds {
  int t[4];
};

__global__ __launch_bounds__(IN_TPB) void in_decide_kernel(const long long* __restrict__ pdesc, const u8* __restrict__ gt,
                                                           const long long* __restrict__ gdesc, const u8* __restrict__ group,
                                                           const u8* __restrict__ things, const int* __restrict__ parea,
                                                           const int* __restrict__ garea, const u64* __restrict__ slot,
                                                           const u32* __restrict__ inter, InThresholds thr, int* __restrict__ pmatch,
                                                           int* __restrict__ gmatch, int* __restrict__ ginter, u64* __restrict__ records,
                                                           int per_image, long long pext, long long gext) {
  __shared__ u8 lut[256], th[256];
  __shared__ u64 acc[256 * IN_SUMS];
  __shared__ int any;
  const int tid = threadIdx.x, b = blockIdx.y;
  lut[tid] = group[tid];
  th[tid] = tid != 255 && things[tid] != 0;
#pragma unroll
  for (int f = 0; f < IN_SUMS; ++f) acc[f * 256 + tid] = 0;
  if (tid == 0) any = 0;
  __syncthreads();
  const InImage im = in_image(pdesc, gdesc, b, pext, gext);
  if (!im.ok) return;
  const long long base = (long long)blockIdx.x * (IN_TPB * IN_STEPS);
  if (base >= im.HW) return;
  for (int k = 0; k < IN_STEPS; ++k) {
    const long long i = base + (long long)k * IN_TPB + tid;
    if (i >= im.HW) break;
    const long long gi = im.goff + i;
    int m = -2, shared_px = 0;
    const int ga = garea[gi];
    if (ga > 0) {
      const int g = lut[gt[gi]];
      if (th[g]) {
        m = -1;
        const u32 cand = in_candidate(slot[gi]);
        if (cand != IN_NONE && (long long)cand < im.HW) {
          const u64 n = inter[gi], pa = (u64)(u32)parea[im.poff + cand];
          if (3 * n > pa + (u64)ga) {
            const u64 uni = pa + (u64)ga - n;
            m = (int)cand;
            shared_px = (int)n;
            pmatch[im.poff + cand] = (int)i;                                   // the one partner of `cand`: no other writer
            u64* a = acc + g * IN_SUMS;
            atomicAdd(&a[0], 1ull);
            atomicAdd(&a[1], (n << 30) / uni);
            atomicAdd(&a[2], n);
            atomicAdd(&a[3], uni);
#pragma unroll
            for (int t = 0; t < 4; ++t)
              if (thr.t[t] && n * 1000ull >= (u64)thr.t[t] * uni) atomicAdd(&a[4 + t], 1ull);
            any = 1;
          }
        }
      }
    }
    gmatch[gi] = m;
    ginter[gi] = shared_px;
  }
  __syncthreads();
  if (!any) return;
  u64* rec = records + (size_t)(per_image ? b : 0) * 256 * IN_FIELDS + (size_t)tid * IN_FIELDS;
#pragma unroll
  for (int f = 0; f < IN_SUMS; ++f) {
    const u64 v = acc[tid * IN_SUMS + f];
    if (v) atomicAdd(&rec[2 + f], v);
  }
}

// ------------------------------------------------------------------------------------------------------------ C ABI
// rows [0, B) of a host table, each acceptable to lm_host_image (labelmap_common.h) -> pixels of the largest image, bytes
// spanned
static int in_scan(const char* who, const char* what, const long* desc_host, int B, long long* max_hw, long long* extent) {
  *max_hw = *extent = 0;
  for (int b = 0; b < B; ++b) {
    long long off, H, W;
    if (int rc = lm_host_image(who, what, desc_host, b, &off, &H, &W)) return rc;
    *max_hw = H * W > *max_hw ? H * W : *max_hw;
    *extent = off + H * W > *extent ? off + H * W : *extent;
  }
  return 0;
}

// both halves of the [2][B][4] host table, and that they agree on every size
static int in_tables(const char* who, const long* desc_host, int B, long long* max_hw, long long* pext, long long* gext) {
  long long ghw;
  if (int rc = in_scan(who, "predicted ", desc_host, B, max_hw, pext)) return rc;
  if (int rc = in_scan(who, "ground-truth ", desc_host + 4 * (size_t)B, B, &ghw, gext)) return rc;
  return lm_host_same_sizes(who, desc_host, B);
}

static inline unsigned in_steps(long long max_hw) { return (unsigned)((max_hw + IN_TPB * IN_STEPS - 1) / (IN_TPB * IN_STEPS)); }

extern "C" size_t hrseg_instances_workspace_bytes(const long* desc_host, int B) {
  const char* who = "hrseg_instances_workspace_bytes";
  if (!desc_host || B < 1 || B > 65535) {
    hrseg_set_error("%s: bad arguments", who);
    return 0;
  }
  long long hw, gext;
  if (in_scan(who, "ground-truth ", desc_host + 4 * (size_t)B, B, &hw, &gext)) return 0;
  return (size_t)gext * 8 + (((size_t)gext * 4 + 7) & ~(size_t)7);
}

extern "C" int hrseg_mask_void_labels(const unsigned char* pred, const long* pdesc, const unsigned char* gt, const long* gdesc,
                                      const long* desc_host, const unsigned char* group, int void_value, unsigned char* out, int B,
                                      hrseg_stream_t stream) {
  const char* who = "hrseg_mask_void_labels";
  HRSEG_CHECK_ARG(pred && pdesc && gt && gdesc && desc_host && group && out, "%s: null pointer", who);
  HRSEG_CHECK_ARG(B >= 1 && B <= 65535, "%s: B=%d not in 1..65535", who, B);
  HRSEG_CHECK_ARG(void_value >= -1 && void_value <= 255, "%s: void_value %d is neither a byte nor -1", who, void_value);
  long long hw, pext, gext;
  if (int rc = in_tables(who, desc_host, B, &hw, &pext, &gext)) return rc;
  HRSEG_CHECK_ARG((uintptr_t)out + (uintptr_t)pext <= (uintptr_t)pred || (uintptr_t)pred + (uintptr_t)pext <= (uintptr_t)out,
                  "%s: out overlaps pred", who);
  hipLaunchKernelGGL(in_mask_kernel, dim3(in_steps(hw), (unsigned)B), dim3(IN_TPB), 0, (hipStream_t)stream, pred, (const long long*)pdesc, gt,
                     (const long long*)gdesc, group, void_value, out, pext, gext);
  HRSEG_LAUNCH_CHECK("mask_void_labels");
  hrseg_count(CNT_SCORE_INSTANCES, HRSEG_MASK_VOID_LABELS_LAUNCHES);
  return 0;
}

extern "C" int hrseg_score_instances(const unsigned char* pm, const long* pdesc, const int* proots, const int* parea,
                                     const unsigned char* gt, const long* gdesc, const int* groots, const int* garea,
                                     const long* desc_host, const unsigned char* group, const unsigned char* things,
                                     const int* thresholds, long long* records, int* pmatch, int* gmatch, int* ginter, void* workspace,
                                     int B, int per_image, hrseg_stream_t stream) {
  const char* who = "hrseg_score_instances";
  HRSEG_CHECK_ARG(pm && pdesc && proots && parea && gt && gdesc && groots && garea && desc_host && group && things && thresholds && records &&
                      pmatch && gmatch && ginter && workspace,
                  "%s: null pointer", who);
  HRSEG_CHECK_ARG(B >= 1 && B <= 65535, "%s: B=%d not in 1..65535", who, B);
  HRSEG_CHECK_ARG((((uintptr_t)proots | (uintptr_t)parea | (uintptr_t)groots | (uintptr_t)garea | (uintptr_t)pmatch | (uintptr_t)gmatch |
                    (uintptr_t)ginter) & 3) == 0,
                  "%s: roots, areas, pmatch, gmatch and ginter must be 4-byte aligned", who);
  HRSEG_CHECK_ARG(((uintptr_t)records & 7) == 0 && ((uintptr_t)workspace & 7) == 0, "%s: records and workspace must be 8-byte aligned", who);
  InThresholds thr;
  for (int t = 0; t < 4; ++t) {
    thr.t[t] = thresholds[t];
    HRSEG_CHECK_ARG(thr.t[t] == 0 || (thr.t[t] >= 501 && thr.t[t] <= 1000), "%s: thresholds[%d]=%d is neither 0 nor in 501..1000", who, t,
                    thr.t[t]);
  }
  long long hw, pext, gext;
  if (int rc = in_tables(who, desc_host, B, &hw, &pext, &gext)) return rc;
  u64* slot = (u64*)workspace;
  u32* inter = (u32*)(slot + gext);
  const hipStream_t st = (hipStream_t)stream;
  const long long* pd = (const long long*)pdesc;
  const long long* gd = (const long long*)gdesc;
  u64* rec = (u64*)records;
  const dim3 steps(in_steps(hw), (unsigned)B), block(IN_TPB);
  const dim3 chunks((unsigned)((hw + IN_WAVES * IN_CHUNK - 1) / (IN_WAVES * IN_CHUNK)), (unsigned)B);
  hipLaunchKernelGGL(in_init_kernel, steps, block, 0, st, pm, pd, gt, gd, group, things, parea, garea, slot, inter, pmatch, rec, per_image,
                     pext, gext);
  HRSEG_LAUNCH_CHECK("score_instances (init)");
  hipLaunchKernelGGL(in_walk_kernel<false>, chunks, block, 0, st, pm, pd, gt, gd, group, things, proots, groots, slot, inter, pext, gext);
  HRSEG_LAUNCH_CHECK("score_instances (vote)");
  hipLaunchKernelGGL(in_walk_kernel<true>, chunks, block, 0, st, pm, pd, gt, gd, group, things, proots, groots, slot, inter, pext, gext);
  HRSEG_LAUNCH_CHECK("score_instances (count)");
  hipLaunchKernelGGL(in_decide_kernel, steps, block, 0, st, pd, gt, gd, group, things, parea, garea, (const u64*)slot, (const u32*)inter, thr,
                     pmatch, gmatch, ginter, rec, per_image, pext, gext);
  HRSEG_LAUNCH_CHECK("score_instances (decide)");
  hrseg_count(CNT_SCORE_INSTANCES, HRSEG_SCORE_INSTANCES_CALL_LAUNCHES);
  return 0;
}
