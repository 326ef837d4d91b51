// lane.hip - the library's lanes: library-owned streams beside the step's, one fork / join path for all of them.
//
// Lane 0, the weight-gradient lane: the batched weight gradients (csrc/gemm_tn.hip) are ~500 us of MFMA work that nothing
// reads before the optimiser, while the embed backward that follows them on the caller's stream is a chain of small
// latency-bound launches.
// Lane 1, the side lane: short chains of latency-bound launches whose neighbours on the step's stream are independent of them
// and bound by another resource (the weight-only prologue beside the HBM-bound embed forward, the classification head beside
// the de-embed GEMM, the first conv's gradients beside the weight-only chain of the embed backward).
// A lane is ONE library-owned stream per device (non-blocking, default priority) plus a fork and a done event.
// dpot_lane_fork orders the lane behind the caller's stream and hands out its handle, dpot_lane_join orders the caller behind
// the lane; between the two the caller sends any launch of the library to the handle (ops.wgrad_flush_async, ops.side_lane).
// Inside a stream capture the event record / wait pair pulls the lane into the capture as a parallel branch; a lane is never
// CREATED there (a first use under capture runs on the caller's stream).  The only state the library keeps; every access is
// under the mutex.
#include "common.h"
#include <mutex>

namespace dpot {
constexpr int LANE_MAXDEV = 64;
constexpr int LANE_COUNT = 2;       // the step's stream plus these: never more than three streams live at once
struct Lane {
  hipStream_t stream;
  hipEvent_t fork, done;
  int pending;          // forks since the last join
  bool ready, captured; // captured: the last fork was made inside a stream capture
};
static Lane g_lane[LANE_COUNT][LANE_MAXDEV];
static std::mutex g_lane_mutex;

static int lane_hip(hipError_t e, const char* what) {
  if (e == hipSuccess) return DPOT_OK;
  (void)hipGetLastError();
  set_error("lane: %s: %s", what, hipGetErrorString(e));
  return DPOT_EHIP;
}
static Lane* lane_of_current_device(int lane = 0) {
  int dev = -1;
  if (lane < 0 || lane >= LANE_COUNT) return nullptr;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= LANE_MAXDEV) { (void)hipGetLastError(); return nullptr; }
  return &g_lane[lane][dev];
}
static bool stream_capturing(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); return true; }   // unknown: treat as capturing
  return st != hipStreamCaptureStatusNone;
}
// The stream is created at the DEFAULT priority.  Measured on the DPOT-Tiny step (profiles/wgrad_lane_ab.txt): with the lane at
// the lowest or at the highest priority of the device's range the replay of the captured step takes twice as long (6.3 ms
// against 2.93 ms; in the kernel trace the lane's first launch starts ~200 us after the fork and the step's own launches fall
// behind as well - cause inside the runtime's graph replay, not looked into), so there is no priority to choose.
static int lane_create(Lane* L) {
  if (L->ready) return DPOT_OK;
  int rc;
  Lane n{};
  rc = lane_hip(hipStreamCreateWithPriority(&n.stream, hipStreamNonBlocking, 0), "hipStreamCreateWithPriority");
  if (rc) return rc;
  rc = lane_hip(hipEventCreateWithFlags(&n.fork, hipEventDisableTiming), "hipEventCreateWithFlags");
  if (!rc) {
    rc = lane_hip(hipEventCreateWithFlags(&n.done, hipEventDisableTiming), "hipEventCreateWithFlags");
    if (rc) (void)hipEventDestroy(n.fork);
  }
  if (rc) { (void)hipStreamDestroy(n.stream); return rc; }
  n.ready = true;
  *L = n;
  return DPOT_OK;
}
// (mutex held)  Order L behind `caller`; *forked = false when L does not exist and may not be created (a first use inside a
// stream capture): the work then belongs on the caller's own stream and nothing is counted.
static int lane_fork_locked(Lane* L, hipStream_t caller, bool* forked) {
  *forked = false;
  const bool capturing = stream_capturing(caller);
  if (!L->ready) {
    if (capturing) return DPOT_OK;
    int rc = lane_create(L);
    if (rc) return rc;
  }
  int rc = lane_hip(hipEventRecord(L->fork, caller), "hipEventRecord(fork)");
  if (rc) return rc;
  rc = lane_hip(hipStreamWaitEvent(L->stream, L->fork, 0), "hipStreamWaitEvent(fork)");
  if (rc) return rc;
  L->pending += 1;
  L->captured = capturing;
  *forked = true;
  return DPOT_OK;
}
// (mutex held)  Order `caller` behind everything L has been given; clears the count.  Nothing when nothing is pending.
static int lane_join_locked(Lane* L, hipStream_t caller) {
  if (!L || !L->ready || L->pending == 0) return DPOT_OK;
  const bool capturing = stream_capturing(caller);
  if (L->captured && !capturing) {   // the capture the fork belonged to has ended or was abandoned: nothing left to order
    L->pending = 0;
    return DPOT_OK;
  }
  DPOT_REQUIRE(L->captured == capturing, "lane: a fork outside a capture cannot be joined inside one");
  int rc = lane_hip(hipEventRecord(L->done, L->stream), "hipEventRecord(done)");
  if (rc) return rc;
  rc = lane_hip(hipStreamWaitEvent(caller, L->done, 0), "hipStreamWaitEvent(done)");
  if (rc) return rc;
  L->pending = 0;
  return DPOT_OK;
}
static int lane_shutdown_locked(Lane* L) {
  if (!L || !L->ready) return DPOT_OK;
  DPOT_REQUIRE(L->pending == 0, "lane: shutdown with %d forks not joined", L->pending);
  int rc = lane_hip(hipStreamSynchronize(L->stream), "hipStreamSynchronize");
  if (rc) return rc;
  (void)hipEventDestroy(L->fork);
  (void)hipEventDestroy(L->done);
  (void)hipStreamDestroy(L->stream);
  *L = Lane{};
  return DPOT_OK;
}
}  // namespace dpot

using namespace dpot;

extern "C" int dpot_lane_init(int lane) {
  std::lock_guard<std::mutex> lock(g_lane_mutex);
  DPOT_REQUIRE(lane >= 0 && lane < LANE_COUNT, "lane: no lane %d", lane);
  Lane* L = lane_of_current_device(lane);
  DPOT_REQUIRE(L, "lane: no current device");
  return lane_create(L);
}

extern "C" int dpot_lane_ready(int lane) {
  std::lock_guard<std::mutex> lock(g_lane_mutex);
  Lane* L = lane_of_current_device(lane);
  return L && L->ready ? 1 : 0;
}

extern "C" int dpot_lane_pending(int lane) {
  std::lock_guard<std::mutex> lock(g_lane_mutex);
  Lane* L = lane_of_current_device(lane);
  return L ? L->pending : 0;
}

extern "C" int dpot_lane_shutdown(int lane) {
  std::lock_guard<std::mutex> lock(g_lane_mutex);
  DPOT_REQUIRE(lane >= 0 && lane < LANE_COUNT, "lane: no lane %d", lane);
  return lane_shutdown_locked(lane_of_current_device(lane));
}

extern "C" int dpot_lane_fork(int lane, dpot_stream_t caller, dpot_stream_t* lane_stream) {
  std::lock_guard<std::mutex> lock(g_lane_mutex);
  DPOT_REQUIRE(lane >= 0 && lane < LANE_COUNT, "lane: no lane %d", lane);
  DPOT_REQUIRE(lane_stream, "lane: fork without a place for the stream handle");
  *lane_stream = caller;
  Lane* L = lane_of_current_device(lane);
  DPOT_REQUIRE(L, "lane: no current device");
  bool forked = false;
  int rc = lane_fork_locked(L, as_stream(caller), &forked);
  if (!rc && forked) *lane_stream = (dpot_stream_t)L->stream;
  return rc;
}

extern "C" int dpot_lane_join(int lane, dpot_stream_t caller) {
  std::lock_guard<std::mutex> lock(g_lane_mutex);
  DPOT_REQUIRE(lane >= 0 && lane < LANE_COUNT, "lane: no lane %d", lane);
  return lane_join_locked(lane_of_current_device(lane), as_stream(caller));
}
