// ggrs_amd/csrc/liveness_step.hpp — one endpoint's receive timers for one poll
// (include/ggrs_amd.h rb_p2p_poll_liveness): UdpProtocol::handle_message's stamp and
// NetworkResumed (network/protocol.rs:555-562), on_input's disconnect_requested (:621-626) and
// poll's two timers (:377-394), over plain values.  Plain C++, no device include:
// p2p_liveness_kernel (liveness.hpp) and the host check (tests/check_liveness.cpp) share it.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RB_LIVENESS_HD __host__ __device__
#else
#define RB_LIVENESS_HD
#endif

namespace rb {

// GGRSEvent::NetworkInterrupted / NetworkResumed / Disconnected (include/ggrs_amd.h RB_NET_*)
constexpr int32_t kLvNone = 0, kLvInterrupted = 1, kLvResumed = 2, kLvDisconnected = 3;
// the endpoint's flags: disconnect_notify_sent, disconnect_event_sent (protocol.rs:140-141)
constexpr uint32_t kLvNotifySent = 1u << 0, kLvEventSent = 1u << 1;
// last_recv_time of an endpoint that has not met a poll yet
constexpr int64_t kLvUnstamped = -1;

// The events one poll can raise, a bit each, bit k before bit k + 1: NetworkResumed
// (handle_message), Disconnected (on_input), NetworkInterrupted, Disconnected (the timers).  At
// most three are set: the two Disconnected share disconnect_event_sent.
constexpr int kLvSlots = 4;
constexpr uint32_t kLvEvResumed = 1u << 0, kLvEvRequested = 1u << 1, kLvEvInterrupted = 1u << 2, kLvEvTimedOut = 1u << 3;
RB_LIVENESS_HD constexpr int32_t liveness_event_kind(int slot) {
  return slot == 0 ? kLvResumed : slot == 2 ? kLvInterrupted : kLvDisconnected;
}

struct LivenessStep {
  int64_t stamp;    // last_recv_time after the poll, ms
  uint32_t flags;   // kLv*Sent after the poll
  uint32_t events;  // kLvEv*, raised in bit order
  int32_t value;    // NetworkInterrupted's disconnect_timeout - disconnect_notify_start (the others carry 0)
};

// One poll of a running endpoint at `now`.  received: a message of any kind came since the last
// poll; requested: an Input message among them carried disconnect_requested.  Both comparisons are
// strict, as the reference's; 64-bit, so no stamp + delay wraps.
RB_LIVENESS_HD inline LivenessStep liveness_step(int64_t stamp, uint32_t flags, bool received, bool requested, int64_t now,
                                                 int32_t notify_start_ms, int32_t timeout_ms) {
  LivenessStep r{stamp, flags, 0u, timeout_ms - notify_start_ms};
  // UdpProtocol::new stamps at construction (:260); here the clock starts at the first poll
  if (r.stamp == kLvUnstamped) r.stamp = now;
  if (received) {  // handle_message (:555-562)
    r.stamp = now;
    if (r.flags & kLvNotifySent) {
      r.flags &= ~kLvNotifySent;
      r.events |= kLvEvResumed;
    }
  }
  if (requested && !(r.flags & kLvEventSent)) {  // on_input (:621-626)
    r.flags |= kLvEventSent;
    r.events |= kLvEvRequested;
  }
  if (!(r.flags & kLvNotifySent) && r.stamp + notify_start_ms < now) {  // poll (:377-386)
    r.flags |= kLvNotifySent;
    r.events |= kLvEvInterrupted;
  }
  if (!(r.flags & kLvEventSent) && r.stamp + timeout_ms < now) {  // poll (:388-394)
    r.flags |= kLvEventSent;
    r.events |= kLvEvTimedOut;
  }
  return r;
}

}  // namespace rb
