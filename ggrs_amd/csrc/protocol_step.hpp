// ggrs_amd/csrc/protocol_step.hpp — one endpoint's share of rb_endpoint_protocol_poll_all
// (include/ggrs_amd.h): the part of the reference's UdpProtocol
// (network/protocol.rs) that decides which message is due and when, over plain values: the state
// machine Initializing -> Synchronizing -> Running -> Disconnected -> Shutdown (:119-125), the sync
// handshake (synchronize :335-341, on_sync_request :578-583, on_sync_reply :586-614), the send
// timers of poll (:351-404), send_input's gate (:444-446) and queue_message's counters (:527-538).
// Plain C++, no device include: the kernel (protocol.hip) and the host check
// (tests/check_protocol.cpp) call the same function; memory is the caller's business.
//
// Nothing here indexes an array with a value that comes from a tensor: the nonce ring, the caller's
// nonces and the outgoing slots are walked with constant indices and selects, so a corrupt state
// row selects among the same registers as a sound one.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RB_PR_HD __host__ __device__ __forceinline__
#define RB_PR_UNROLL _Pragma("unroll")
#else
#define RB_PR_HD inline __attribute__((always_inline))
#define RB_PR_UNROLL
#endif

namespace rb {

// ProtocolState (protocol.rs:119-125); include/ggrs_amd.h RB_EP_*
constexpr uint32_t kEpInitializing = 0, kEpSynchronizing = 1, kEpRunning = 2, kEpDisconnected = 3, kEpShutdown = 4;
constexpr int32_t kPrSyncPackets = 5;         // NUM_SYNC_PACKETS (network/mod.rs)
constexpr int64_t kPrShutdownTimer = 5000;    // UDP_SHUTDOWN_TIMER, protocol.rs:20
constexpr int64_t kPrInterval = 200;          // SYNC_RETRY / RUNNING_RETRY / KEEP_ALIVE / QUALITY_REPORT_INTERVAL, :22-25
constexpr int kPrNonces = 8;                  // the outstanding nonces kept per endpoint
constexpr int kPrMaxSlots = 8;                // RB_DG_MAX_SLOTS
constexpr int kPrSyncBytes = 10;              // magic u16, variant u32, nonce u32
constexpr uint32_t kPrSyncRequest = 0, kPrSyncReply = 1;  // MessageBody's variants, messages.rs:82-92
constexpr uint32_t kPrNoRoom = 32;            // RB_DG_NO_ROOM
constexpr uint32_t kPrEvSynchronizing = 1, kPrEvSynchronized = 2;

struct PrState {  // one row of every state tensor; a fresh endpoint is all zero
  uint32_t state;
  int32_t sync_remaining;
  uint32_t nonces[kPrNonces];
  uint32_t valid, next;  // one bit per entry of nonces; the entry the next insert writes
  int64_t last_send, last_input_recv, last_quality_report, shutdown_at, stats_start;
  int64_t packets_sent;
  int32_t last_newest;  // newest + 1 of the last Input declared due (0: none yet)
  uint32_t remote_magic;
};

struct PrInput {  // what the caller hands in for one endpoint and call
  int64_t now;
  uint32_t local_magic;
  uint32_t start, disconnected, ack_owed, reply_owed, received;  // zero / non-zero
  int32_t newest, acked, length;
  int32_t reports;     // the session's checksum reports of this poll
  int32_t slots, sync_slots;
  uint32_t tag[kPrMaxSlots];     // pr_digest of every incoming slot: 0, or kPrTagSync | variant << 16 | magic
  uint32_t x[kPrMaxSlots];       // the sync message's u32
  uint32_t nonces[kPrMaxSlots];   // the caller's randomness: request j of this call uses nonces[j], j < slots
};

struct PrOutput {
  int32_t input_length;
  uint32_t ack_due, reply_due, report_due, keepalive_due;
  uint32_t msg[kPrMaxSlots][3];  // the sync messages, 10 bytes each
  int32_t sync_msgs;
  uint32_t events;
  int32_t sync_count;
  uint32_t liveness_received;
  int32_t send_queue_len;
  uint32_t synchronized;  // is_synchronized(), protocol.rs:307-311
  uint32_t status;
};

// An incoming slot, from avail = min(length, stride) and its first 12 bytes w: a sync message has at
// least 10 bytes and variant 0 or 1 (only those two kinds are read here; bytes at or above avail
// decide nothing).
constexpr uint32_t kPrTagSync = 1u << 31;
RB_PR_HD void pr_digest(int32_t avail, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t& tag, uint32_t& x) {
  const uint32_t variant = (w0 >> 16) | (w1 << 16);
  const bool sync = avail >= kPrSyncBytes && variant <= kPrSyncReply;
  tag = sync ? kPrTagSync | (variant << 16) | (w0 & 0xFFFFu) : 0u;
  x = sync ? (w1 >> 16) | (w2 << 16) : 0u;
}

// stamp + delay < now, strict and in 64 bits; a corrupt stamp wraps instead of overflowing
RB_PR_HD bool pr_after(int64_t stamp, int64_t delay, int64_t now) {
  return static_cast<int64_t>(static_cast<uint64_t>(stamp) + static_cast<uint64_t>(delay)) < now;
}

// a where pick, else b, as arithmetic: the optimiser turns a chain of selects over an array back
// into an indexed access of memory, and this it leaves in registers
RB_PR_HD uint32_t pr_pick(bool pick, uint32_t a, uint32_t b) {
  const uint32_t m = 0u - static_cast<uint32_t>(pick);
  return (a & m) | (b & ~m);
}

// A SyncRequest / SyncReply as bincode lays it out: magic u16 | variant u32 | u32
RB_PR_HD void pr_sync_message(uint32_t magic, uint32_t variant, uint32_t x, uint32_t (&w)[3]) {
  w[0] = (magic & 0xFFFFu) | (variant << 16);  // the variant's upper bytes are zero
  w[1] = x << 16;
  w[2] = x >> 16;
}

// queue_message for a sync message: the next outgoing slot, or RB_DG_NO_ROOM
RB_PR_HD bool pr_emit(const PrInput& in, PrOutput& out, uint32_t variant, uint32_t x) {
  if (out.sync_msgs >= in.sync_slots) {
    out.status |= kPrNoRoom;
    return false;
  }
  uint32_t w[3];
  pr_sync_message(in.local_magic, variant, x, w);
  RB_PR_UNROLL
  for (int m = 0; m < kPrMaxSlots; ++m) {
    const bool here = out.sync_msgs == m;
    RB_PR_UNROLL
    for (int i = 0; i < 3; ++i) out.msg[m][i] = pr_pick(here, w[i], out.msg[m][i]);
  }
  ++out.sync_msgs;
  return true;
}

// send_sync_request (protocol.rs:507-514): the caller's next nonce joins the outstanding ones.  A
// request that finds no slot, or no nonce left, is not sent and not recorded.
RB_PR_HD void pr_send_sync_request(PrState& st, const PrInput& in, PrOutput& out, int32_t& requests) {
  if (requests >= in.slots) {
    out.status |= kPrNoRoom;
    return;
  }
  uint32_t x = 0;
  RB_PR_UNROLL
  for (int j = 0; j < kPrMaxSlots; ++j) x = pr_pick(requests == j, in.nonces[j], x);
  if (!pr_emit(in, out, kPrSyncRequest, x)) return;
  ++requests;
  bool held = false;  // HashSet::insert of a value already there adds nothing
  RB_PR_UNROLL
  for (int i = 0; i < kPrNonces; ++i) held = held || (((st.valid >> i) & 1u) && st.nonces[i] == x);
  if (held) return;
  const uint32_t at = st.next & (kPrNonces - 1);
  RB_PR_UNROLL
  for (int i = 0; i < kPrNonces; ++i) st.nonces[i] = pr_pick(at == static_cast<uint32_t>(i), x, st.nonces[i]);
  st.valid = (st.valid | (1u << at)) & 0xFFu;
  st.next = (at + 1u) & (kPrNonces - 1);
}

RB_PR_HD void pr_clear(PrOutput& out) {
  out.input_length = 0;
  out.ack_due = out.reply_due = out.report_due = out.keepalive_due = 0u;
  RB_PR_UNROLL
  for (int m = 0; m < kPrMaxSlots; ++m) out.msg[m][0] = out.msg[m][1] = out.msg[m][2] = 0u;
  out.sync_msgs = 0;
  out.events = 0u;
  out.sync_count = 0;
  out.send_queue_len = 0;
  out.status = 0u;
  out.liveness_received = out.synchronized = 0u;
}

// Steps 2 to 9 for an endpoint that is not in Shutdown
RB_PR_HD void pr_run(PrState& st, const PrInput& in, PrOutput& out) {
  pr_clear(out);
  const int64_t now = in.now;
  int32_t requests = 0;
  int32_t due = 0;  // messages declared due so far, sync messages apart

  // disconnect(), :325-333
  if (in.disconnected && st.state != kEpDisconnected) {
    st.state = kEpDisconnected;
    st.shutdown_at = static_cast<int64_t>(static_cast<uint64_t>(now) + static_cast<uint64_t>(kPrShutdownTimer));
  }
  // synchronize(), :335-341; the three stamps of the constructor (:226-260) are taken here
  if (in.start && st.state == kEpInitializing) {
    st.state = kEpSynchronizing;
    st.sync_remaining = kPrSyncPackets;
    st.stats_start = now;
    st.last_send = st.last_input_recv = st.last_quality_report = now;
    pr_send_sync_request(st, in, out, requests);
  }
  // handle_message (:544-575) for the two sync kinds, in slot order
  RB_PR_UNROLL
  for (int m = 0; m < kPrMaxSlots; ++m) {
    if (m >= in.slots || !(in.tag[m] & kPrTagSync)) continue;
    const uint32_t magic = in.tag[m] & 0xFFFFu, variant = (in.tag[m] >> 16) & 1u, x = in.x[m];
    if (st.remote_magic != 0u && magic != st.remote_magic) continue;  // :551
    if (variant == kPrSyncRequest) {  // on_sync_request, :578-583
      pr_emit(in, out, kPrSyncReply, x);
      continue;
    }
    if (st.state != kEpSynchronizing) continue;  // on_sync_reply, :586-614
    uint32_t hit = 0;
    RB_PR_UNROLL
    for (int i = 0; i < kPrNonces; ++i) hit |= (((st.valid >> i) & 1u) && st.nonces[i] == x) ? 1u << i : 0u;
    if (hit == 0u) continue;
    st.valid &= ~hit;
    st.sync_remaining = static_cast<int32_t>(static_cast<uint32_t>(st.sync_remaining) - 1u);
    if (st.sync_remaining > 0) {
      out.events |= kPrEvSynchronizing;
      pr_send_sync_request(st, in, out, requests);
    } else {
      st.state = kEpRunning;
      out.events |= kPrEvSynchronized;
      st.remote_magic = magic;
    }
  }
  // what the caller's parse and decode owe: send_input_ack with on_input's stamp (:654, :682),
  // on_quality_report's reply (:697-701)
  if (in.ack_owed) {
    out.ack_due = 1u;
    st.last_input_recv = now;
    ++due;
  }
  if (in.reply_owed) {
    out.reply_due = 1u;
    ++due;
  }
  // poll's timers, :351-404.  queue_message stamps last_send_time at once (:533), so a message
  // already declared due in this call holds the timers that read it.
  bool input_due = false;
  bool shut = false;
  if (st.state == kEpSynchronizing) {
    if (out.sync_msgs + due == 0 && pr_after(st.last_send, kPrInterval, now)) pr_send_sync_request(st, in, out, requests);
  } else if (st.state == kEpRunning) {
    if (pr_after(st.last_input_recv, kPrInterval, now)) {
      st.last_input_recv = now;
      input_due = in.newest > in.acked;  // send_pending_output with a front, :468-471
    }
    if (pr_after(st.last_quality_report, kPrInterval, now)) {
      st.last_quality_report = now;
      out.report_due = 1u;
      ++due;
    }
  } else if (st.state == kEpDisconnected) {
    if (pr_after(st.shutdown_at, 0, now)) {
      st.state = kEpShutdown;
      shut = true;
    }
  }
  // the frame's own sends: send_input in Running only (:444-446), the checksum reports (:736-742)
  const int32_t newest1 = in.newest < 0 ? 0 : in.newest == INT32_MAX ? INT32_MAX : in.newest + 1;
  if (newest1 > st.last_newest) {
    input_due = input_due || st.state == kEpRunning;
    st.last_newest = newest1;
  }
  if (input_due) {
    out.input_length = in.length;
    ++due;
  }
  due += in.reports;
  // send_keep_alive, :372-375
  if (st.state == kEpRunning && out.sync_msgs + due == 0 && pr_after(st.last_send, kPrInterval, now)) {
    out.keepalive_due = 1u;
    ++due;
  }
  out.sync_count = static_cast<int32_t>(static_cast<uint32_t>(kPrSyncPackets) - static_cast<uint32_t>(st.sync_remaining));
  const int64_t queue = static_cast<int64_t>(in.newest) - in.acked;
  out.send_queue_len = queue <= 0 ? 0 : queue > INT32_MAX ? INT32_MAX : static_cast<int32_t>(queue);
  if (shut) {  // the queue is drained before the socket sees it, :429-432
    out.input_length = 0;
    out.ack_due = out.reply_due = out.report_due = out.keepalive_due = 0u;
    out.sync_msgs = 0;
    due = 0;
  }
  // queue_message's counters, :527-538
  const int32_t sent = out.sync_msgs + due;
  st.packets_sent = static_cast<int64_t>(static_cast<uint64_t>(st.packets_sent) + static_cast<uint64_t>(sent));
  if (sent > 0) st.last_send = now;
}

// One endpoint, one call.  Returns false for an endpoint in Shutdown (or in no known state), which
// reads nothing and sends nothing (send_all_messages :429-432, handle_message :546-548): its state
// rows are not to be written.  `out` is complete either way.
RB_PR_HD bool pr_step(PrState& st, const PrInput& in, PrOutput& out) {
  const bool live = st.state < kEpShutdown;
  if (live) pr_run(st, in, out);
  else pr_clear(out);
  out.liveness_received = (st.state != kEpRunning || in.received) ? 1u : 0u;
  out.synchronized = st.state >= kEpRunning ? 1u : 0u;
  return live;
}

}  // namespace rb
