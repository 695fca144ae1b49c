// ggrs_amd/csrc/protocol.hip — UdpProtocol's handshake, state machine and send timers for every
// endpoint of a batch in one launch (include/ggrs_amd.h rb_endpoint_protocol_poll_all, DESIGN.md
// section 20).  The per-endpoint step is protocol_step.hpp's, shared with tests/check_protocol.cpp;
// this file owns the layout, the loads and the stores.
//
// One lane per session: it walks the handles of the mask in ascending order, the loop unrolled over
// the player count the kernel is instantiated for, so session_running has one writer and nothing
// needs an atomic or LDS.  A wave holds 64 consecutive sessions, so its accesses to one field of
// one handle are one row.  Every load whose address the lane knows, for every handle, is issued
// before the first store; no address depends on a byte of a datagram or of a state row.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <type_traits>

#include "../../include/ggrs_amd.h"
#include "protocol_step.hpp"

namespace {

using namespace rb;

static_assert(kEpInitializing == RB_EP_INITIALIZING && kEpSynchronizing == RB_EP_SYNCHRONIZING && kEpRunning == RB_EP_RUNNING &&
                  kEpDisconnected == RB_EP_DISCONNECTED && kEpShutdown == RB_EP_SHUTDOWN,
              "header and step agree");
static_assert(kPrMaxSlots == RB_DG_MAX_SLOTS && kPrNoRoom == RB_DG_NO_ROOM && kPrEvSynchronizing == RB_EP_EVENT_SYNCHRONIZING &&
                  kPrEvSynchronized == RB_EP_EVENT_SYNCHRONIZED,
              "header and step agree");
constexpr int kThreads = 64;  // one wave: the kernel holds a call's whole input in registers

struct ProtocolParams {
  rb_endpoint_protocol io;
  int32_t S;
  uint32_t mask;
};

template <int P>
__global__ void __launch_bounds__(kThreads) endpoint_protocol_kernel(const ProtocolParams p) {
  const int s = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= p.S) return;
  const rb_endpoint_protocol& io = p.io;
  const size_t S = static_cast<size_t>(p.S), PS = static_cast<size_t>(P) * S;

  // the session's checksum reports of this poll, read once
  int32_t reports = 0;
  if (io.reports) {
#pragma unroll
    for (int k = 0; k < RB_P2P_REPORTS_PER_TAKE; ++k) reports += io.reports[static_cast<size_t>(k) * S + s].frame != RB_NULL_FRAME ? 1 : 0;
  }

  // every handle's state rows, caller's bytes and datagram heads, before the first store (the
  // branches on the mask, the slot count and the optional tensors are uniform)
  PrState st[P];
  PrInput in[P];
#pragma unroll
  for (int h = 0; h < P; ++h) {
    if (!((p.mask >> h) & 1u)) continue;
    const size_t e = static_cast<size_t>(h) * S + s;
    PrState& t = st[h];
    t.state = io.ep_state[e];
    t.sync_remaining = io.sync_remaining[e];
#pragma unroll
    for (int i = 0; i < kPrNonces; ++i) t.nonces[i] = io.sync_nonces[static_cast<size_t>(i) * PS + e];
    t.valid = io.sync_valid[e];
    t.next = io.sync_next[e];
    t.last_send = io.stamps[e];
    t.last_input_recv = io.stamps[PS + e];
    t.last_quality_report = io.stamps[2 * PS + e];
    t.shutdown_at = io.stamps[3 * PS + e];
    t.stats_start = io.stamps[4 * PS + e];
    t.packets_sent = io.packets_sent[e];
    t.last_newest = io.last_newest[e];
    t.remote_magic = io.remote_magic[e];
    PrInput& x = in[h];
    x.now = io.now_ms;
    x.local_magic = io.local_magic[e];
    x.start = io.start ? io.start[e] : 0u;
    x.disconnected = io.disconnected ? io.disconnected[e] : 0u;
    x.ack_owed = io.ack_owed ? io.ack_owed[e] : 0u;
    x.reply_owed = io.reply_owed ? io.reply_owed[e] : 0u;
    x.received = io.received ? io.received[e] : 0u;
    x.newest = io.newest[e];
    x.acked = io.acked[e];
    x.length = io.lengths ? io.lengths[e] : 0;
    x.reports = reports;
    x.slots = io.slots;
    x.sync_slots = io.sync_slots;
#pragma unroll
    for (int m = 0; m < kPrMaxSlots; ++m) {
      x.tag[m] = x.x[m] = x.nonces[m] = 0u;
      if (m < io.slots) {
        const size_t row = static_cast<size_t>(m) * PS + e;
        const int32_t len = io.dg_lengths[row];
        // stride >= 16: the 16 bytes are inside the row, whatever the length says
        const uint4 v = *reinterpret_cast<const uint4*>(io.datagrams + static_cast<int64_t>(row) * io.stride);
        pr_digest(len < io.stride ? len : static_cast<int32_t>(io.stride), v.x, v.y, v.z, x.tag[m], x.x[m]);
        x.nonces[m] = io.nonces[row];
      }
    }
  }

  // One handle's step and stores.  Called once per handle below and not from a loop: the body is
  // large, and an unrolling that stopped short would index st and in by a register.
  uint32_t running = 1u;
  auto serve = [&](auto handle) {
    constexpr int h = decltype(handle)::value;
    if (!((p.mask >> h) & 1u)) return;
    const size_t e = static_cast<size_t>(h) * S + s;
    PrState& t = st[h];
    PrOutput o;
    const bool live = pr_step(t, in[h], o);
    running &= o.synchronized;
    if (live) {
      io.ep_state[e] = static_cast<uint8_t>(t.state);
      io.sync_remaining[e] = t.sync_remaining;
#pragma unroll
      for (int i = 0; i < kPrNonces; ++i) io.sync_nonces[static_cast<size_t>(i) * PS + e] = t.nonces[i];
      io.sync_valid[e] = static_cast<uint8_t>(t.valid);
      io.sync_next[e] = static_cast<uint8_t>(t.next);
      io.stamps[e] = t.last_send;
      io.stamps[PS + e] = t.last_input_recv;
      io.stamps[2 * PS + e] = t.last_quality_report;
      io.stamps[3 * PS + e] = t.shutdown_at;
      io.stamps[4 * PS + e] = t.stats_start;
      io.packets_sent[e] = t.packets_sent;
      io.last_newest[e] = t.last_newest;
      io.remote_magic[e] = static_cast<uint16_t>(t.remote_magic);
    }
    io.input_lengths[e] = o.input_length;
    io.ack_due[e] = static_cast<uint8_t>(o.ack_due);
    io.reply_due[e] = static_cast<uint8_t>(o.reply_due);
    io.report_due[e] = static_cast<uint8_t>(o.report_due);
    io.keepalive_due[e] = static_cast<uint8_t>(o.keepalive_due);
#pragma unroll
    for (int m = 0; m < kPrMaxSlots; ++m) {
      if (m >= io.sync_slots) continue;  // uniform
      const size_t row = static_cast<size_t>(m) * PS + e;
      const bool used = m < o.sync_msgs;
      io.sync_lengths[row] = used ? kPrSyncBytes : 0;
      if (used)
        *reinterpret_cast<uint4*>(io.sync_datagrams + static_cast<int64_t>(row) * io.stride) =
            make_uint4(o.msg[m][0], o.msg[m][1], o.msg[m][2], 0u);
    }
    io.sync_counts[e] = o.sync_msgs;
    io.events[e] = static_cast<uint8_t>(o.events);
    io.sync_count[e] = o.sync_count;
    if (io.liveness_received) io.liveness_received[e] = static_cast<uint8_t>(o.liveness_received);
    if (io.send_queue_len) io.send_queue_len[e] = o.send_queue_len;
    io.status[e] = static_cast<int32_t>(o.status);
  };
  serve(std::integral_constant<int, 0>{});
  if constexpr (P > 1) serve(std::integral_constant<int, 1>{});
  if constexpr (P > 2) serve(std::integral_constant<int, 2>{});
  if constexpr (P > 3) serve(std::integral_constant<int, 3>{});
  if (io.session_running) io.session_running[s] = static_cast<uint8_t>(running);
}

// The launch's own status, not the thread's last error: an earlier call's leftover is not this launch's.
template <int P>
rb_status launch(const ProtocolParams& params, hipStream_t stream) {
  ProtocolParams copy = params;
  void* args[] = {&copy};
  const dim3 grid((params.S + kThreads - 1) / kThreads);
  const hipError_t err =
      hipLaunchKernel(reinterpret_cast<const void*>(endpoint_protocol_kernel<P>), grid, dim3(kThreads), args, 0, stream);
  if (err == hipSuccess) return RB_OK;
  std::fprintf(stderr, "rb_endpoint_protocol_poll_all: %s\n", hipGetErrorString(err));
  return RB_DEVICE_ERROR;
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" rb_status rb_endpoint_protocol_poll_all(int32_t device, void* stream, uint32_t handle_mask, int32_t num_players,
                                                   int32_t num_sessions, const rb_endpoint_protocol* io) {
  if (!io || num_players <= 0 || num_players > 4 || num_sessions <= 0) return RB_INVALID_REQUEST;
  if (handle_mask == 0 || (handle_mask >> num_players) != 0) return RB_INVALID_REQUEST;
  if (io->slots < 1 || io->slots > RB_DG_MAX_SLOTS || io->sync_slots < 1 || io->sync_slots > RB_DG_MAX_SLOTS || io->now_ms < 0)
    return RB_INVALID_REQUEST;
  if (io->stride < 16 || io->stride % 16 != 0 || io->stride > (1 << 20)) return RB_INVALID_REQUEST;
  if (!io->datagrams || !io->sync_datagrams || !aligned16(io->datagrams) || !aligned16(io->sync_datagrams))
    return RB_INVALID_REQUEST;
  if (!io->ep_state || !io->sync_remaining || !io->sync_nonces || !io->sync_valid || !io->sync_next || !io->stamps ||
      !io->packets_sent || !io->last_newest || !io->remote_magic || !io->local_magic || !io->dg_lengths || !io->nonces ||
      !io->newest || !io->acked || !io->input_lengths || !io->ack_due || !io->reply_due || !io->report_due ||
      !io->keepalive_due || !io->sync_lengths || !io->sync_counts || !io->events || !io->sync_count || !io->status)
    return RB_INVALID_REQUEST;
  if (const hipError_t err = hipSetDevice(device); err != hipSuccess) {
    std::fprintf(stderr, "hipSetDevice(%d): %s\n", device, hipGetErrorString(err));
    return RB_DEVICE_ERROR;
  }
  const ProtocolParams p{*io, num_sessions, handle_mask};
  hipStream_t q = static_cast<hipStream_t>(stream);
  return num_players == 1 ? launch<1>(p, q) : num_players == 2 ? launch<2>(p, q) : num_players == 3 ? launch<3>(p, q) : launch<4>(p, q);
}
