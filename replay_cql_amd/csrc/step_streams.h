// The streams and events the step driver (train.hip) forks onto and joins by; chosen once per device in step_streams.hip.
#pragma once
#include "common.h"

// Fork/join through events only, so the structure stays capturable in a hipGraph.
struct SideStream {
  hipStream_t st_items = nullptr;    // pair sorts of a step that was not sampled ahead (forward), item-side backward + Adam
  hipStream_t st_branch = nullptr;   // branch B of the forward (s' rows: argmax + target network); encoder dW in the backward
  hipStream_t st_ahead = nullptr;    // sampling + sorts of the NEXT step (cqlrec_train_steps) = cqlrec_aux_stream(0)
  hipEvent_t sorted[2] = {nullptr, nullptr};   // sorted pairs of the step with this parity are in place
  hipEvent_t forked = nullptr, fork2 = nullptr, join2 = nullptr;
  hipEvent_t loss = nullptr, items_done = nullptr, dh = nullptr, eout = nullptr, presample = nullptr, fwd_done = nullptr;
  hipEvent_t read_map = nullptr;   // the read map of the step sampled ahead is in place (the E_in optimizer waits for it)
  bool ok = false;                 // all three streams and every event exist; false: serial mode, everything on the caller's
  bool tried = false;
};

// this device's set (created on first use); never ok while concurrency is off (cqlrec_set_concurrency, CQL_CONCURRENCY=0)
SideStream& side_stream();
