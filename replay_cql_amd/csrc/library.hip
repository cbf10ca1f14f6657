// The library itself: last-error text, ABI version, measurement hooks, parameter layout.  Host code only.
#include "common.h"

// =============================================================================================================
// error plumbing
// =============================================================================================================
static thread_local char g_err[512] = "";
void cql_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* cqlrec_last_error(void) { return g_err; }
extern "C" int cqlrec_abi_version(void) { return CQLREC_ABI_VERSION; }

// =============================================================================================================
// measurement hooks: event pairs around kernels, on the launching stream
// =============================================================================================================
#define CQL_PROF_POOL 8192
static struct {
  bool on = false;
  bool created = false;
  hipEvent_t ev[CQL_PROF_POOL][2];
  int phase[CQL_PROF_POOL];
  int n = 0;
  int open = -1;
  uint32_t mask = 0xFFFFFFFFu;   // phases that are bracketed while on
} g_prof;

void cql_prof_begin(int phase, hipStream_t s) {
  if (!g_prof.on || g_prof.n >= CQL_PROF_POOL || !((g_prof.mask >> phase) & 1u)) return;
  g_prof.open = g_prof.n++;
  g_prof.phase[g_prof.open] = phase;
  (void)hipEventRecord(g_prof.ev[g_prof.open][0], s);
}
void cql_prof_end(hipStream_t s) {
  if (!g_prof.on || g_prof.open < 0) return;
  (void)hipEventRecord(g_prof.ev[g_prof.open][1], s);
  g_prof.open = -1;
}
extern "C" int cqlrec_prof_select(uint32_t phase_mask) {
  g_prof.mask = phase_mask;
  return CQLREC_OK;
}
extern "C" int cqlrec_prof_enable(int32_t on) {
  if (on && !g_prof.created) {
    for (int i = 0; i < CQL_PROF_POOL; ++i)
      for (int k = 0; k < 2; ++k)
        if (hipEventCreate(&g_prof.ev[i][k]) != hipSuccess) {
          cql_set_error("prof_enable: hipEventCreate failed");
          return CQLREC_ERR_HIP;
        }
    g_prof.created = true;
  }
  g_prof.on = on != 0;
  g_prof.n = 0;
  g_prof.open = -1;
  return CQLREC_OK;
}
extern "C" int cqlrec_prof_read(double* ms_sum, int64_t* launches) {
  CQL_REQUIRE(ms_sum && launches, "prof_read: NULL pointer");
  for (int p = 0; p < CQLREC_PH_COUNT; ++p) {
    ms_sum[p] = 0.0;
    launches[p] = 0;
  }
  for (int i = 0; i < g_prof.n; ++i) {
    float ms = 0.f;
    if (hipEventSynchronize(g_prof.ev[i][1]) != hipSuccess ||
        hipEventElapsedTime(&ms, g_prof.ev[i][0], g_prof.ev[i][1]) != hipSuccess) {
      cql_set_error("prof_read: event query failed");
      return CQLREC_ERR_HIP;
    }
    ms_sum[g_prof.phase[i]] += ms;
    launches[g_prof.phase[i]] += 1;
  }
  g_prof.n = 0;
  return CQLREC_OK;
}

extern "C" int cqlrec_layout_make(int64_t n_items, int32_t d, cqlrec_layout* out) {
  CQL_REQUIRE(out != nullptr, "layout_make: out is NULL");
  CQL_REQUIRE(n_items > 0 && n_items < (1ll << 31) - 64, "layout_make: n_items=%lld out of range", (long long)n_items);
  CQL_REQUIRE(cql_d_ok(d), "layout_make: d=%d unsupported (64, 128 or 256)", d);
  int64_t sizes[7] = {(n_items + 1) * d, n_items * d, n_items, (int64_t)d * d, d, (int64_t)d * d, d};
  int64_t offs[7], cur = 0;
  for (int i = 0; i < 7; ++i) {
    offs[i] = cur;
    cur += (sizes[i] + CQLREC_SEG_ALIGN - 1) / CQLREC_SEG_ALIGN * CQLREC_SEG_ALIGN;
  }
  out->n_items = n_items;
  out->d = d;
  out->reserved = 0;
  out->off_E_in = offs[0];
  out->off_E_out = offs[1];
  out->off_b_out = offs[2];
  out->off_W1 = offs[3];
  out->off_b1 = offs[4];
  out->off_W2 = offs[5];
  out->off_b2 = offs[6];
  out->total = cur;
  return CQLREC_OK;
}
