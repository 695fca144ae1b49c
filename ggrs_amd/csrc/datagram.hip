// ggrs_amd/csrc/datagram.hip — GGRS's wire messages for every endpoint of a batch in one launch
// (include/ggrs_amd.h rb_parse_datagrams_all / rb_build_datagrams_all):
// UdpProtocol::handle_message (network/protocol.rs:544-575) over the datagrams the caller's sockets
// collected, and the messages queue_message's callers build (:468-525, :736-742).  The per-endpoint
// steps are datagram_step.hpp's, shared with tests/check_datagram.cpp; this file owns the layout,
// the loads and the stores.
//
// One lane per endpoint, handle-major as in wire.hip: blockIdx.y walks the handles of the mask, a
// wave holds 64 consecutive sessions of one handle, so its accesses to one field are one row.
// The kernels are instantiated per player count: every field offset of an Input, and the byte
// shift of its payload copy, is then a constant, and a datagram's head is read from registers
// with constant indices only.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../include/ggrs_amd.h"
#include "datagram_step.hpp"

namespace {

using namespace rb;

static_assert(kDgReportsKept == RB_P2P_REPORTS_PER_TAKE && kDgMaxSlots == RB_DG_MAX_SLOTS, "header and step agree");
static_assert(kDgMalformed == RB_DG_MALFORMED && kDgMagicMismatch == RB_DG_MAGIC_MISMATCH && kDgSyncSeen == RB_DG_SYNC_SEEN &&
                  kDgBadPong == RB_DG_BAD_PONG && kDgReportsDropped == RB_DG_REPORTS_DROPPED && kDgNoRoom == RB_DG_NO_ROOM &&
                  kDgAdvantageRange == RB_DG_ADVANTAGE_RANGE,
              "header and step agree");

__host__ inline uint32_t pack_handles(uint32_t mask, int& count) {  // the handles of a mask, one per byte, lowest first
  uint32_t packed = 0;
  count = 0;
  for (uint32_t h = 0; h < 4; ++h)
    if ((mask >> h) & 1u) packed |= h << (8 * count++);
  return packed;
}

__device__ __forceinline__ DgChunk load16(const uint8_t* row, int32_t c) {
  const uint4 v = reinterpret_cast<const uint4*>(row)[c];
  return DgChunk{{v.x, v.y, v.z, v.w}};
}
__device__ __forceinline__ void store16(uint8_t* row, int32_t c, const DgChunk& x) {
  reinterpret_cast<uint4*>(row)[c] = make_uint4(x.w[0], x.w[1], x.w[2], x.w[3]);
}

struct ParseParams {
  rb_datagram_parse io;
  int32_t S;
  uint32_t handles;  // pack_handles
};

template <int P>
__global__ void __launch_bounds__(256) parse_datagrams_kernel(const ParseParams p) {
  using Y = DgLayout<P>;
  constexpr int HW = Y::kHeadWords;
  const int s = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= p.S) return;
  const rb_datagram_parse& io = p.io;
  const int h = static_cast<int>((p.handles >> (8 * blockIdx.y)) & 0xFFu);
  const size_t S = static_cast<size_t>(p.S), PS = static_cast<size_t>(P) * S, e = static_cast<size_t>(h) * S + s;
  // every load whose address the lane knows, before the first store: the lengths and heads of all
  // slots, the magic and the in/out words
  int32_t lens[kDgMaxSlots];
  uint32_t heads[kDgMaxSlots][HW];
#pragma unroll
  for (int m = 0; m < kDgMaxSlots; ++m) {
    lens[m] = 0;
#pragma unroll
    for (int i = 0; i < HW; ++i) heads[m][i] = 0u;
    if (m < io.slots) {  // uniform
      const size_t row = static_cast<size_t>(m) * PS + e;
      lens[m] = io.dg_lengths[row];
      const uint8_t* d = io.datagrams + static_cast<int64_t>(row) * io.stride;  // stride >= 64: the head is inside the row
#pragma unroll
      for (int c = 0; c < HW / 4; ++c) {
        const DgChunk x = load16(d, c);
#pragma unroll
        for (int i = 0; i < 4; ++i) heads[m][4 * c + i] = x.w[i];
      }
    }
  }
  const uint32_t magic = io.remote_magic[e];
  const int32_t count_in = io.report_counts[e];
  DgEndpoint ep = dg_endpoint(io.acked[e], io.frame_advantage[e], io.rtt_ms[e]);

  // handle_message per slot, in slot order, from registers
#pragma unroll
  for (int m = 0; m < kDgMaxSlots; ++m) {
    if (lens[m] <= 0) continue;
    const int32_t avail = lens[m] < io.stride ? lens[m] : static_cast<int32_t>(io.stride);
    dg_parse_one<P>(heads[m], avail, m, magic, io.now_ms, ep);
  }
  const DgReportPlan plan = dg_report_plan(count_in, dg_popcount8(ep.report_slots));
  if (plan.drop > 0) ep.status |= kDgReportsDropped;

  io.received[e] = static_cast<uint8_t>(ep.received);
  io.disconnect_requested[e] = static_cast<uint8_t>(ep.disconnect_requested);
  io.acked[e] = ep.acked;
  io.frame_advantage[e] = ep.frame_advantage;
  io.rtt_ms[e] = ep.rtt_ms;
  io.reply_owed[e] = static_cast<uint8_t>(ep.reply_owed);
  io.reply_ping[e] = ep.ping_lo;
  io.reply_ping[PS + e] = ep.ping_hi;
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const size_t at = (static_cast<size_t>(h) * P + i) * S + s;
    io.peer_last_frames[at] = ep.peer_last[i];
    io.peer_disconnected[at] = static_cast<uint8_t>((ep.peer_disconnected >> i) & 1u);
  }
  io.lengths[e] = ep.input_slot >= 0 ? ep.payload_len : 0;
  io.start_frames[e] = ep.input_slot >= 0 ? ep.start_frame : 0;
  io.report_counts[e] = plan.count;
  io.status[e] = static_cast<int32_t>(ep.status);

  // the checksum reports: the kept ones move down past the dropped (rare), the fresh ones follow
  // from their heads, the rest is cleared
  rb_checksum_report* const rep = io.reports + static_cast<size_t>(h) * kDgReportsKept * S + s;
  for (int32_t j = 0; j + plan.drop < plan.kept; ++j) rep[static_cast<size_t>(j) * S] = rep[static_cast<size_t>(j + plan.drop) * S];
  int32_t pos = plan.kept - plan.drop;
#pragma unroll
  for (int m = 0; m < kDgMaxSlots; ++m) {
    if (!((ep.report_slots >> m) & 1u)) continue;
    const DgReport r = dg_report_of<HW>(heads[m]);  // pos >= 0: at most 8 fresh reports, so drop <= kept
    rep[static_cast<size_t>(pos) * S] = rb_checksum_report{r.lo, r.hi, r.frame, RB_NULL_FRAME};
    ++pos;
  }
  for (int32_t j = plan.count; j < kDgReportsKept; ++j)
    rep[static_cast<size_t>(j) * S] = rb_checksum_report{0u, 0u, RB_NULL_FRAME, RB_NULL_FRAME};

  // the last Input's payload, from byte 31 + 5 P of its datagram, into the packet row: 16-byte loads
  // through a shifting two-chunk window, 16-byte stores.  The parse bounded payload_len by the
  // datagram's bytes; the row takes its first packet_stride.
  if (ep.input_slot >= 0 && ep.payload_len > 0) {
    const uint8_t* d = io.datagrams + static_cast<int64_t>(static_cast<size_t>(ep.input_slot) * PS + e) * io.stride;
    uint8_t* out = io.packets + static_cast<int64_t>(e) * io.packet_stride;
    const int32_t n = ep.payload_len < io.packet_stride ? ep.payload_len : static_cast<int32_t>(io.packet_stride);
    dg_copy_from<Y::kPayload>([&](int32_t c) { return load16(d, c); }, (Y::kPayload + ep.payload_len + 15) >> 4, n,
                              [&](int32_t c, const DgChunk& x) { store16(out, c, x); });
  }
}

struct BuildParams {
  rb_datagram_build io;
  int32_t S;
  uint32_t handles;
};

template <int P>
__global__ void __launch_bounds__(256) build_datagrams_kernel(const BuildParams p) {
  const int s = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= p.S) return;
  const rb_datagram_build& io = p.io;
  const int h = static_cast<int>((p.handles >> (8 * blockIdx.y)) & 0xFFu);
  const size_t S = static_cast<size_t>(p.S), PS = static_cast<size_t>(P) * S, e = static_cast<size_t>(h) * S + s;
  // everything the endpoint owes, loaded before the first store (the optional tensors' branches are uniform)
  DgOwed o{};
  o.magic = io.local_magic[e];
  o.now_ms = io.now_ms;
  o.ack_frame = io.ack_frame[e];
  if (io.packets) {
    o.input_len = io.lengths[e];
    o.start_frame = io.start_frames[e];
  }
  if (io.disconnect_requested) o.disconnect_requested = io.disconnect_requested[e];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    o.status_last[i] = io.status_last_frames[static_cast<size_t>(i) * S + s];
    o.status_disconnected |= (io.status_disconnected[static_cast<size_t>(i) * S + s] ? 1u : 0u) << i;
  }
  if (io.ack_owed) o.ack_owed = io.ack_owed[e];
  if (io.reply_owed) {
    o.reply_owed = io.reply_owed[e];
    o.ping_lo = io.reply_ping[e];
    o.ping_hi = io.reply_ping[PS + e];
  }
  if (io.report_due) {
    o.report_due = io.report_due[e];
    o.frame_advantage = io.frame_advantage[e];
  }
  if (io.keepalive_due) o.keepalive_due = io.keepalive_due[e];
#pragma unroll
  for (int k = 0; k < kDgReportsKept; ++k) {
    o.reports[k] = DgReport{0u, 0u, kDgNullFrame};
    if (io.reports) {
      const rb_checksum_report r = io.reports[static_cast<size_t>(k) * S + s];
      o.reports[k] = DgReport{r.checksum_lo, r.checksum_hi, r.frame};
    }
  }
  uint32_t status = 0;
  if (io.packets && o.input_len > io.packet_stride) {  // the row does not hold that many bytes
    status |= kDgMalformed;
    o.input_len = 0;
  }
  const uint8_t* pk = io.packets + static_cast<int64_t>(e) * io.packet_stride;
  auto row = [&](int32_t slot) -> uint8_t* {
    return io.out_datagrams + static_cast<int64_t>(static_cast<size_t>(slot) * PS + e) * io.stride;
  };
  const int32_t count = dg_build_endpoint<P>(
      o, io.slots, io.stride, status,
      [&](int32_t slot, int32_t bytes) {
        io.out_lengths[static_cast<size_t>(slot) * PS + e] = bytes;
        uint8_t* out = row(slot);
        dg_emit_input<P>(o, [&](int32_t c) { return load16(pk, c); }, [&](int32_t c, const DgChunk& x) { store16(out, c, x); });
      },
      [&](int32_t slot, const DgFixed& m) {
        io.out_lengths[static_cast<size_t>(slot) * PS + e] = m.len;
        uint8_t* out = row(slot);  // stride >= 64: both chunks are inside the row
        store16(out, 0, DgChunk{{m.w[0], m.w[1], m.w[2], m.w[3]}});
        store16(out, 1, DgChunk{{m.w[4], m.w[5], m.w[6], m.w[7]}});
      });
  for (int32_t slot = count; slot < io.slots; ++slot) io.out_lengths[static_cast<size_t>(slot) * PS + e] = 0;
  io.out_counts[e] = count;
  io.status[e] = static_cast<int32_t>(status);
}

bool shape_ok(uint32_t handle_mask, int32_t num_players, int32_t num_sessions, const void* datagrams, int64_t stride,
              int32_t slots, int64_t now_ms) {
  if (num_players <= 0 || num_players > 4 || num_sessions <= 0) return false;
  if (handle_mask == 0 || (handle_mask >> num_players) != 0) return false;
  if (slots < 1 || slots > RB_DG_MAX_SLOTS || now_ms < 0) return false;
  if (!datagrams || stride < 64 || stride % 16 != 0 || stride > (1 << 20) || reinterpret_cast<uintptr_t>(datagrams) % 16 != 0)
    return false;
  return true;
}

bool packets_ok(const void* packets, int64_t packet_stride) {
  return packet_stride >= 32 && packet_stride % 16 == 0 && packet_stride <= (1 << 20) &&
         reinterpret_cast<uintptr_t>(packets) % 16 == 0;
}

// The launch's own status, not the thread's last error: an earlier call's leftover is not this launch's.
template <class Params>
rb_status launch(void (*kernel)(const Params), dim3 grid, hipStream_t stream, const Params& params, const char* what) {
  Params copy = params;
  void* args[] = {&copy};
  const hipError_t err = hipLaunchKernel(reinterpret_cast<const void*>(kernel), grid, dim3(256), args, 0, stream);
  if (err == hipSuccess) return RB_OK;
  std::fprintf(stderr, "%s: %s\n", what, hipGetErrorString(err));
  return RB_DEVICE_ERROR;
}

#define RB_LAUNCH_BY_PLAYERS(kernel, players, grid, stream, params, what)                      \
  ((players) == 1   ? launch(kernel<1>, grid, stream, params, what)                            \
   : (players) == 2 ? launch(kernel<2>, grid, stream, params, what)                            \
   : (players) == 3 ? launch(kernel<3>, grid, stream, params, what)                            \
                    : launch(kernel<4>, grid, stream, params, what))

}  // namespace

extern "C" {

rb_status rb_parse_datagrams_all(int32_t device, void* stream, uint32_t handle_mask, int32_t num_players,
                                 int32_t num_sessions, const rb_datagram_parse* io) {
  if (!io || !shape_ok(handle_mask, num_players, num_sessions, io->datagrams, io->stride, io->slots, io->now_ms))
    return RB_INVALID_REQUEST;
  if (!io->packets || !packets_ok(io->packets, io->packet_stride)) return RB_INVALID_REQUEST;
  if (!io->dg_lengths || !io->remote_magic || !io->received || !io->disconnect_requested || !io->acked ||
      !io->peer_last_frames || !io->peer_disconnected || !io->lengths || !io->start_frames || !io->frame_advantage ||
      !io->reply_owed || !io->reply_ping || !io->rtt_ms || !io->reports || !io->report_counts || !io->status)
    return RB_INVALID_REQUEST;
  if (const hipError_t err = hipSetDevice(device); err != hipSuccess) {
    std::fprintf(stderr, "hipSetDevice(%d): %s\n", device, hipGetErrorString(err));
    return RB_DEVICE_ERROR;
  }
  int count = 0;
  const uint32_t handles = pack_handles(handle_mask, count);
  const ParseParams p{*io, num_sessions, handles};
  const dim3 grid((num_sessions + 255) / 256, count);
  return RB_LAUNCH_BY_PLAYERS(parse_datagrams_kernel, num_players, grid, static_cast<hipStream_t>(stream), p,
                              "rb_parse_datagrams_all");
}

rb_status rb_build_datagrams_all(int32_t device, void* stream, uint32_t handle_mask, int32_t num_players,
                                 int32_t num_sessions, const rb_datagram_build* io) {
  if (!io || !shape_ok(handle_mask, num_players, num_sessions, io->out_datagrams, io->stride, io->slots, io->now_ms))
    return RB_INVALID_REQUEST;
  if (io->packets && (!packets_ok(io->packets, io->packet_stride) || !io->lengths || !io->start_frames))
    return RB_INVALID_REQUEST;
  if (!io->local_magic || !io->ack_frame || !io->status_last_frames || !io->status_disconnected || !io->out_lengths ||
      !io->out_counts || !io->status || (io->reply_owed && !io->reply_ping) || (io->report_due && !io->frame_advantage))
    return RB_INVALID_REQUEST;
  if (const hipError_t err = hipSetDevice(device); err != hipSuccess) {
    std::fprintf(stderr, "hipSetDevice(%d): %s\n", device, hipGetErrorString(err));
    return RB_DEVICE_ERROR;
  }
  int count = 0;
  const uint32_t handles = pack_handles(handle_mask, count);
  const BuildParams p{*io, num_sessions, handles};
  const dim3 grid((num_sessions + 255) / 256, count);
  return RB_LAUNCH_BY_PLAYERS(build_datagrams_kernel, num_players, grid, static_cast<hipStream_t>(stream), p,
                              "rb_build_datagrams_all");
}

}  // extern "C"
