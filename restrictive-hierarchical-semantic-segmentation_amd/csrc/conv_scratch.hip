// Scratch ring and persistent weight-image cache of the convolution dispatch (conv.hip): where the pre-split weight images
// of the wave-specialised and halo-patch bodies live, and which of them are rebuilt per launch.  Self-contained host state
// with its own ABI calls (hrseg_set_scratch, hrseg_set_weight_image_arena, hrseg_weight_images_refresh); the dispatcher sees
// scratch_usable / scratch_reserve / ws_make_images (conv_common.h).  No kernels here: the image kernels are conv_ws.hip's,
// launched through launch_weight_images / launch_weight_image_table.
#include "conv_common.h"
#include <mutex>
#include <vector>

// ---- scratch ring (hrseg_set_scratch)
// The pre-split weight images live in a scratch buffer the host hands over once (hrseg_set_scratch; device memory is
// the caller's, as everywhere in this ABI).  It is cut into eight regions, one per stream that launches convolutions,
// each a ring: an image is written and read by kernels of ONE stream, in order, so reusing a slot after the ring
// wraps needs no synchronisation.  Without a scratch buffer the path is simply not taken.
static unsigned char* g_scratch = nullptr;
static size_t g_scratch_bytes = 0;
static int g_scratch_device = -1;       // the device that was current when the buffer was attached: launches on another one do not use it
static std::mutex g_scratch_mu;         // the region table is the only mutable state the launch path shares between host threads
struct ScratchRegion { hipStream_t st; bool used; size_t head; };
static const int SCRATCH_REGIONS = 8;
static ScratchRegion g_regions[SCRATCH_REGIONS];
extern "C" int hrseg_set_scratch(void* ptr, size_t bytes) {
  HRSEG_CHECK_ARG((ptr && bytes >= (1u << 20)) || (!ptr && bytes == 0), "hrseg_set_scratch: need a buffer of at least 1 MiB, or (null, 0)");
  HRSEG_CHECK_ARG(((uintptr_t)ptr & 255) == 0, "hrseg_set_scratch: the buffer must be 256-byte aligned");
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  g_scratch = (unsigned char*)ptr;
  g_scratch_bytes = bytes;
  g_scratch_device = -1;
  if (ptr && hipGetDevice(&g_scratch_device) != hipSuccess) g_scratch_device = -1;
  for (auto& r : g_regions) r = ScratchRegion{nullptr, false, 0};
  return 0;
}
bool scratch_usable() {
  if (!g_scratch) return false;
  int dev = -1;
  return hipGetDevice(&dev) == hipSuccess && dev == g_scratch_device;
}
// `bytes` CONTIGUOUS bytes of this stream's ring.  All images of one grouped launch are reserved together: they are written by one
// kernel and read by the next, so a wrap between two of them would put a later image over an earlier one of the same launch.
// nullptr: no buffer (or one of another device), no free region for a ninth stream, or more than a region holds.
unsigned char* scratch_reserve(hipStream_t st, size_t bytes) {
  if (!scratch_usable()) return nullptr;
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  const size_t region = (g_scratch_bytes / SCRATCH_REGIONS) & ~(size_t)255;
  bytes = (bytes + 255) & ~(size_t)255;
  if (bytes > region) return nullptr;
  int r = -1;
  for (int i = 0; i < SCRATCH_REGIONS && r < 0; ++i)
    if (g_regions[i].used && g_regions[i].st == st) r = i;
  for (int i = 0; i < SCRATCH_REGIONS && r < 0; ++i)
    if (!g_regions[i].used) { g_regions[i] = ScratchRegion{st, true, 0}; r = i; }
  if (r < 0) return nullptr;
  if (g_regions[r].head + bytes > region) g_regions[r].head = 0;       // wrap BEFORE the group, never inside it
  unsigned char* p = g_scratch + (size_t)r * region + g_regions[r].head;
  g_regions[r].head += bytes;
  return p;
}
// ---- persistent weight images (hrseg_set_weight_image_arena / hrseg_weight_images_refresh) ------------------------------
// A weight image depends on the weights alone, and those change once per step: instead of one small image launch in front
// of every convolution (136 per HRNet step, 5.5 us + a kernel boundary each, all on the critical path) the images of the
// model's parameters live in an arena the caller owns and are rebuilt by ONE launch when the caller says the weights
// changed.  An image is cached only for a weight the caller flags as persistent (hrseg_conv_shape_t.w_persistent) AND that
// lies inside one of the two registered source ranges (the flat parameter buffer and its transposed copy): a scratch tensor
// that happens to reuse a dead model's addresses never hits.  First use of a weight registers it (and builds its image on
// the spot, as before); every later refresh rebuilds all registered images.  Single-threaded like the rest of the launch path.
struct ImgEntry { const float* w; unsigned char* img; int K, N, layout, ns, nblk; float wscale; };
static std::vector<ImgEntry> g_img;
static unsigned char* g_img_arena = nullptr;
static size_t g_img_arena_bytes = 0, g_img_arena_head = 0;
static WeightImageTabEntry* g_img_tab = nullptr;       // device copy of g_img for the refresh kernel (caller's memory)
static size_t g_img_tab_cap = 0;
static bool g_img_dirty = false;
static const float* g_img_range[4] = {nullptr, nullptr, nullptr, nullptr};
static int g_img_device = -1;
extern "C" int hrseg_set_weight_image_arena(void* arena, size_t bytes, void* table, size_t table_bytes, const float* lo0,
                                            const float* hi0, const float* lo1, const float* hi1) {
  HRSEG_CHECK_ARG((arena && bytes >= (1u << 20) && table && table_bytes >= sizeof(WeightImageTabEntry)) || (!arena && bytes == 0),
                  "hrseg_set_weight_image_arena: need an arena of at least 1 MiB and a table, or (null, 0)");
  HRSEG_CHECK_ARG((((uintptr_t)arena | (uintptr_t)table) & 255) == 0, "hrseg_set_weight_image_arena: buffers must be 256-byte aligned");
  g_img.clear();
  g_img_arena = (unsigned char*)arena;
  g_img_arena_bytes = bytes;
  g_img_arena_head = 0;
  g_img_tab = (WeightImageTabEntry*)table;
  g_img_tab_cap = arena ? table_bytes / sizeof(WeightImageTabEntry) : 0;
  g_img_dirty = false;
  g_img_range[0] = lo0; g_img_range[1] = hi0; g_img_range[2] = lo1; g_img_range[3] = hi1;
  g_img_device = -1;
  if (arena && hipGetDevice(&g_img_device) != hipSuccess) g_img_device = -1;
  return 0;
}
static bool img_cacheable(const IgemmArgs& a) {
  if (!g_img_arena || !a.w_persistent) return false;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != g_img_device) return false;
  return (a.w >= g_img_range[0] && a.w < g_img_range[1]) || (a.w >= g_img_range[2] && a.w < g_img_range[3]);
}
extern "C" int hrseg_weight_images_refresh(hrseg_stream_t stream) {
  if (g_img.empty()) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (g_img_dirty) {
    std::vector<WeightImageTabEntry> tab(g_img.size());
    int end = 0;
    for (size_t i = 0; i < g_img.size(); ++i) {
      end += g_img[i].nblk;
      tab[i] = WeightImageTabEntry{g_img[i].w, g_img[i].img, g_img[i].K, g_img[i].layout, g_img[i].ns, end, g_img[i].wscale, 0};
    }
    // (pageable source: the call returns once the table is staged; only after new weights were registered)
    if (hipMemcpyAsync(g_img_tab, tab.data(), tab.size() * sizeof(WeightImageTabEntry), hipMemcpyHostToDevice, st) != hipSuccess)
    { hrseg_set_error("hrseg_weight_images_refresh: table upload failed"); return HRSEG_ERR_LAUNCH; }
    g_img_dirty = false;
  }
  int total = 0;
  for (const auto& e : g_img) total += e.nblk;
  launch_weight_image_table(g_img_tab, (int)g_img.size(), total, st);
  HRSEG_LAUNCH_CHECK("weight_image_table");
  return 0;
}
// the weight images of n problems (sets a[i].wimg): cached ones are used as they are, the others are written with one launch
// (into their new arena slot, or into this stream's scratch ring); false: no scratch space
bool ws_make_images(IgemmArgs* a, const int* kinds, int n, hipStream_t st, int ns) {
  WeightImageGroup g;
  g.n = 0;
  g.ns = ns;
  size_t off[MAXG], total = 0;
  int build[MAXG], nb = 0;
  unsigned char* dst[MAXG];
  for (int i = 0; i < n; ++i) {
    dst[i] = nullptr;
    const int layout = kinds[i] == 4 ? 1 : kinds[i];        // kinds 1 and 4 share the (48, 48) image layout
    const size_t bytes = (ws_image_bytes(a[i], kinds[i], ns) + 255) & ~(size_t)255;
    if (img_cacheable(a[i])) {
      for (const auto& e : g_img)
        if (e.w == a[i].w && e.layout == layout && e.ns == ns && e.K == a[i].K && e.N == a[i].N && e.wscale == a[i].wscale) { dst[i] = e.img; break; }
      if (dst[i]) continue;                                  // cached: kept current by hrseg_weight_images_refresh
      if (g_img_arena_head + bytes <= g_img_arena_bytes && g_img.size() < g_img_tab_cap) {
        const int wtn = WS_WTN[kinds[i]], cs = WS_CS[kinds[i]];
        dst[i] = g_img_arena + g_img_arena_head;
        g_img_arena_head += bytes;
        g_img.push_back(ImgEntry{a[i].w, dst[i], a[i].K, a[i].N, layout, ns, (a[i].N / (16 * wtn)) * (a[i].K / (16 * cs)) * ((9 * cs + 1) / 2),
                                 a[i].wscale});
        g_img_dirty = true;
        build[nb++] = i;
        continue;
      }
    }
    off[i] = total;
    total += bytes;
    build[nb++] = i;
  }
  unsigned char* base = total ? scratch_reserve(st, total) : nullptr;
  if (total && !base) return false;
  int end = 0;
  for (int j = 0; j < nb; ++j) {
    const int i = build[j];
    if (!dst[i]) dst[i] = base + off[i];
    const int wtn = WS_WTN[kinds[i]], cs = WS_CS[kinds[i]];
    end += (a[i].N / (16 * wtn)) * (a[i].K / (16 * cs)) * ((9 * cs + 1) / 2);
    g.blk_end[g.n] = end;
    g.kind[g.n] = kinds[i];
    g.K[g.n] = a[i].K;
    g.wscale[g.n] = a[i].wscale;
    g.w[g.n] = a[i].w;
    g.img[g.n] = dst[i];
    ++g.n;
  }
  for (int i = 0; i < n; ++i) a[i].wimg = dst[i];
  if (g.n) launch_weight_images(g, end, st);
  return true;
}
