// Process-wide state of libhrseg_hip.so that is no kernel's own: the thread-local error string and the ABI version, the launch
// counters (hrseg_launch_count) and the tuning knobs (hrseg_tune).  Families and knobs are the rows of runtime.h.
#include <stdarg.h>
#include <string.h>

#include "common.h"

static thread_local char g_err[512] = "";

void hrseg_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* hrseg_last_error_string(void) { return g_err; }
extern "C" int hrseg_abi_version(void) { return 17; }

// ---- launch counters
long hrseg_g_cnt[CNT_N];
#define HRSEG_X(id, name, conv) {name, conv},
static const struct { const char* name; int in_conv_total; } g_families[CNT_N] = {HRSEG_FAMILIES(HRSEG_X)};
#undef HRSEG_X

extern "C" long hrseg_launch_count(const char* family, int reset) {
  long total = 0;
  for (int i = 0; i < CNT_N; ++i) {
    if (family && strcmp(family, g_families[i].name)) continue;
    if (family || g_families[i].in_conv_total) total += hrseg_g_cnt[i];
    if (reset) hrseg_g_cnt[i] = 0;      // (no family: EVERY counter starts over, counted in the total or not)
  }
  return total;
}

// ---- tuning knobs
#define HRSEG_X(key, def, restore, meaning) int hrseg_g_##key = def;
HRSEG_KNOBS(HRSEG_X)
#undef HRSEG_X
#define HRSEG_X(key, def, restore, meaning) {#key, &hrseg_g_##key, def, restore},
static const struct { const char* key; int* value; int def, restore; } g_knobs[] = {HRSEG_KNOBS(HRSEG_X)};
#undef HRSEG_X

extern "C" int hrseg_tune(const char* key, int value) {
  HRSEG_CHECK_ARG(key != nullptr, "hrseg_tune: null key");
  for (const auto& k : g_knobs)
    if (!strcmp(k.key, key)) {
      *k.value = (k.restore && value <= 0) ? k.def : value;
      return 0;
    }
  hrseg_set_error("hrseg_tune: unknown key '%s'", key);
  return HRSEG_ERR_INVALID_ARG;
}
