// Which streams the training step runs on: the library's three internal streams and the caller's two aux streams are
// picked here, once per device, by a dispatch-conflict test (cqlrec_runtime_init); train.hip only uses them.
#include <stdlib.h>
#include "step_streams.h"

static int g_concurrency = -1;   // -1: read CQL_CONCURRENCY on first use (default on)

// 1 (default): independent parts of the step run on internal side streams (fork/join by events); 0: everything on the
// caller's stream in program order (used for per-kernel timing, where overlapped launches would blur the durations)
extern "C" int cqlrec_set_concurrency(int32_t on) {
  g_concurrency = on ? 1 : 0;
  return CQLREC_OK;
}

namespace {
bool concurrency_on() {
  if (g_concurrency < 0) {
    const char* v = getenv("CQL_CONCURRENCY");
    g_concurrency = (v && *v == '0') ? 0 : 1;
  }
  return g_concurrency != 0;
}
// ---- which streams may run beside each other -----------------------------------------------------------------------------
// Measured on MI355X / ROCm 7.2 (tools/probes/pipe_probe.hip, profiles/r03_pipe_probe.txt): a process's hardware queues sit
// on the 4 compute pipes round-robin in the order in which its streams were first used, and while a grid larger than the
// chip is being handed out on one queue, NO kernel of another queue on the same pipe is dispatched.  The step driver runs
// four streams side by side (the caller's + three); whether two of them share a pipe used to depend on what else the
// process had created streams for, and in which order -- a torch.cuda.Stream() between the log generation and the first
// step, or the model constructed before the first kernel on the default stream, cost the step ALL of its concurrency
// (cfg3: 1.33 instead of 0.69 ms; tools/stream_order_probe3.py).  So the streams are CHOSEN: out of a handful of fresh
// candidates, three that block neither the caller's (default) stream nor each other, by the same two-kernel test.
__global__ __launch_bounds__(64) void cql_pipe_hog_kernel(int spins) {
  extern __shared__ volatile char pad[];      // 60 KiB of dynamic LDS: two blocks per CU resident, the rest of the grid waits
  pad[threadIdx.x] = 1;
  for (int i = 0; i < spins; ++i) __builtin_amdgcn_s_sleep(127);
  pad[threadIdx.x + 64] = pad[threadIdx.x];
}
__global__ void cql_pipe_tiny_kernel() {}

struct PipeProbe {
  hipEvent_t a0 = nullptr, a1 = nullptr, b1 = nullptr;
  bool ok = false;
  PipeProbe() {
    ok = hipEventCreate(&a0) == hipSuccess && hipEventCreate(&a1) == hipSuccess && hipEventCreate(&b1) == hipSuccess;
  }
  ~PipeProbe() {
    for (hipEvent_t e : {a0, a1, b1})
      if (e) (void)hipEventDestroy(e);
  }
  // 1: a kernel on y is not dispatched while a large grid on x is being handed out; 0: it is; -1: the test failed
  int conflict(hipStream_t x, hipStream_t y) {
    if (!ok || hipDeviceSynchronize() != hipSuccess) return -1;
    (void)hipEventRecord(a0, x);
    hipLaunchKernelGGL(cql_pipe_hog_kernel, dim3(8192), dim3(64), 60 * 1024, x, 3);     // ~0.2 ms
    (void)hipEventRecord(a1, x);
    hipLaunchKernelGGL(cql_pipe_tiny_kernel, dim3(1), dim3(64), 0, y);
    (void)hipEventRecord(b1, y);
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return -1;
    float t_hog = 0.f, t_tiny = 0.f;
    if (hipEventElapsedTime(&t_hog, a0, a1) != hipSuccess || hipEventElapsedTime(&t_tiny, a0, b1) != hipSuccess) return -1;
    return (t_hog > 0.02f && t_tiny > 0.5f * t_hog) ? 1 : 0;
  }
};

hipStream_t g_aux[CQL_MAX_DEVICES][CQLREC_AUX_STREAMS] = {};
int g_pick_report[CQL_MAX_DEVICES] = {};     // candidates looked at (0: no probe ran), for cqlrec_runtime_probe_count

// three streams for the step driver + one more for the caller, all first used HERE, in this order
bool pick_streams(hipStream_t main, hipStream_t out[3], hipStream_t* extra, int* looked_at) {
  constexpr int NC = 8;
  static const bool probe_on = !(getenv("CQL_PIPE_PROBE") && getenv("CQL_PIPE_PROBE")[0] == '0');
  hipStream_t cand[NC] = {};
  bool used[NC] = {};
  int n_out = 0;
  *looked_at = 0;
  hipLaunchKernelGGL(cql_pipe_tiny_kernel, dim3(1), dim3(64), 0, main);       // the caller's queue exists first
  PipeProbe pp;
  int made = 0;
  for (; made < NC && n_out < 3; ++made) {
    if (hipStreamCreateWithFlags(&cand[made], hipStreamNonBlocking) != hipSuccess) break;
    hipLaunchKernelGGL(cql_pipe_tiny_kernel, dim3(1), dim3(64), 0, cand[made]);   // binds its queue now: creation order
    bool good = true;
    if (probe_on && pp.ok) {
      *looked_at = made + 1;
      good = pp.conflict(main, cand[made]) == 0;
      for (int k = 0; good && k < n_out; ++k) good = pp.conflict(out[k], cand[made]) == 0;
    }
    if (good) {
      out[n_out++] = cand[made];
      used[made] = true;
    }
  }
  // not enough independent ones (queues exhausted, probe failed): take what there is, as before
  for (int i = 0; i < made && n_out < 3; ++i)
    if (!used[i]) {
      out[n_out++] = cand[i];
      used[i] = true;
    }
  while (n_out < 3) {
    hipStream_t st;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return false;
    out[n_out++] = st;
  }
  // the caller's extra stream: an unused candidate that does not block the caller's main stream, else a fresh one
  *extra = nullptr;
  for (int i = 0; i < made; ++i)
    if (!used[i] && !*extra && (!probe_on || !pp.ok || pp.conflict(main, cand[i]) == 0)) {
      *extra = cand[i];
      used[i] = true;
    }
  for (int i = 0; i < made; ++i)
    if (!used[i]) (void)hipStreamDestroy(cand[i]);
  if (!*extra && hipStreamCreateWithFlags(extra, hipStreamNonBlocking) != hipSuccess) return false;
  return hipDeviceSynchronize() == hipSuccess;
}
}  // namespace

SideStream& side_stream() {
  static SideStream per_device[CQL_MAX_DEVICES];     // streams and events belong to the device they were created on
  static SideStream off;   // never ok: serial mode
  if (!concurrency_on()) return off;
  const int slot = cql_device_slot();
  SideStream& ss = per_device[slot];
  if (!ss.tried) {
    ss.tried = true;
    // Plain streams, all of one priority class (mixing priority classes did not steer the dispatcher).  A data-parallel
    // caller never runs cqlrec_train_steps: ITS item-side stream (cqlrec_aux_stream(0)) is the sample-ahead stream.
    hipStream_t pk[3] = {};
    hipStream_t extra = nullptr;
    ss.ok = pick_streams(nullptr, pk, &extra, &g_pick_report[slot]);
    if (ss.ok) {
      ss.st_branch = pk[0];
      ss.st_items = pk[1];
      ss.st_ahead = pk[2];
      if (!g_aux[slot][0]) g_aux[slot][0] = pk[2];      // (already set: runtime_init ran while the library was in serial mode)
      if (!g_aux[slot][1]) g_aux[slot][1] = extra;
    }
    for (hipEvent_t* e : {&ss.sorted[0], &ss.sorted[1], &ss.forked, &ss.fork2, &ss.join2, &ss.loss, &ss.items_done, &ss.dh,
                          &ss.eout, &ss.presample, &ss.read_map, &ss.fwd_done})
      ss.ok = ss.ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
  }
  return ss;
}

extern "C" int cqlrec_runtime_init(void) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) {
    cql_set_error("runtime_init: no HIP device");
    return CQLREC_ERR_HIP;
  }
  const int slot = cql_device_slot();
  if (concurrency_on()) {
    if (!side_stream().ok) {
      cql_set_error("runtime_init: creating the internal streams failed");
      return CQLREC_ERR_HIP;
    }
  } else {      // strict program order inside the library: the caller's side streams are plain ones
    for (int i = 0; i < CQLREC_AUX_STREAMS; ++i)
      if (!g_aux[slot][i] && hipStreamCreateWithFlags(&g_aux[slot][i], hipStreamNonBlocking) != hipSuccess) {
        cql_set_error("runtime_init: creating aux stream %d failed", i);
        return CQLREC_ERR_HIP;
      }
  }
  return CQLREC_OK;
}

extern "C" int cqlrec_runtime_probe_count(void) { return g_pick_report[cql_device_slot()]; }

extern "C" cqlrec_stream cqlrec_aux_stream(int32_t index) {
  if (index < 0 || index >= CQLREC_AUX_STREAMS) return nullptr;
  return (cqlrec_stream)g_aux[cql_device_slot()][index];
}
