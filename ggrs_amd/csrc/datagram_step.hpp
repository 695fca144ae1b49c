// ggrs_amd/csrc/datagram_step.hpp — one endpoint's share of rb_parse_datagrams_all and
// rb_build_datagrams_all (include/ggrs_amd.h): the reference's
// Message { header: { magic }, body } as bincode 1.3 lays it out (network/messages.rs,
// udp_socket.rs:31-45), UdpProtocol::handle_message (network/protocol.rs:544-575) with on_input's
// head (:616-637), on_input_ack (:692-694), on_quality_report / on_quality_reply (:697-708), and
// the messages queue_message's callers build (:468-525, :736-742), over plain values.
// Plain C++, no device include: the kernels (datagram.hip) and the host check
// (tests/check_datagram.cpp) call the same functions; memory is reached through the caller's
// functors only, so each side brings its own layout and its own bounds.
//
// A datagram: magic u16, variant u32, body.  Fixed-width little-endian integers, a Vec length is a
// u64, a bool one byte that must be 0 or 1.  The Input body for P players:
//   u64 n (== P) | P x (bool disconnected, i32 last_frame) | bool disconnect_requested |
//   i32 start_frame | i32 ack_frame | u64 len | len bytes
// so its payload starts at byte 31 + 5 P.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RB_DG_HD __host__ __device__ __forceinline__
#define RB_DG_UNROLL _Pragma("unroll")
#else
#define RB_DG_HD inline __attribute__((always_inline))
#define RB_DG_UNROLL
#endif

namespace rb {

// MessageBody's variants (messages.rs:82-92)
constexpr uint32_t kDgSyncRequest = 0, kDgSyncReply = 1, kDgInput = 2, kDgInputAck = 3, kDgQualityReport = 4,
                   kDgQualityReply = 5, kDgChecksumReport = 6, kDgKeepAlive = 7;
// status bits (include/ggrs_amd.h RB_DG_*)
constexpr uint32_t kDgMalformed = 1u, kDgMagicMismatch = 2u, kDgSyncSeen = 4u, kDgBadPong = 8u, kDgReportsDropped = 16u,
                   kDgNoRoom = 32u, kDgAdvantageRange = 64u;
constexpr int kDgMaxSlots = 8;     // datagram slots per endpoint and call
constexpr int kDgReportsKept = 8;  // RB_P2P_REPORTS_PER_TAKE
constexpr int32_t kDgNullFrame = -1;
constexpr int kDgHeaderBytes = 6;  // magic, variant

template <int P>
struct DgLayout {
  static_assert(P >= 1 && P <= 4, "one to four players");
  static constexpr int kCount = kDgHeaderBytes;   // u64 n
  static constexpr int kStatus = kCount + 8;      // P x (bool, i32)
  static constexpr int kRequested = kStatus + 5 * P;
  static constexpr int kStart = kRequested + 1;
  static constexpr int kAck = kStart + 4;
  static constexpr int kLen = kAck + 4;           // u64
  static constexpr int kPayload = kLen + 8;       // 31 + 5 P
  // the datagram's head held in registers: every fixed-size kind and Input's fixed part
  static constexpr int kHeadWords = kPayload <= 48 ? 12 : 16;
};

struct DgChunk {  // 16 bytes, byte 0 in the low byte of w[0]
  uint32_t w[4];
};

// bytes r .. r + 3 of the eight bytes (lo, hi), r in 0..3
RB_DG_HD uint32_t dg_funnel(uint32_t lo, uint32_t hi, int r) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, static_cast<uint32_t>(r));
#else
  return r == 0 ? lo : (lo >> (8 * r)) | (hi << (32 - 8 * r));
#endif
}

// fields of a head at a byte offset the caller knows at compile time
template <int HW>
RB_DG_HD uint32_t dg_u32(const uint32_t (&w)[HW], int off) {
  const int i = off >> 2;
  return dg_funnel(w[i], i + 1 < HW ? w[i + 1] : 0u, off & 3);
}
template <int HW>
RB_DG_HD uint32_t dg_u8(const uint32_t (&w)[HW], int off) {
  return (w[off >> 2] >> (8 * (off & 3))) & 0xFFu;
}
template <int HW>
RB_DG_HD uint64_t dg_u64(const uint32_t (&w)[HW], int off) {
  return static_cast<uint64_t>(dg_u32(w, off)) | (static_cast<uint64_t>(dg_u32(w, off + 4)) << 32);
}
template <int HW>
RB_DG_HD void dg_put_u32(uint32_t (&w)[HW], int off, uint32_t v) {
  const int i = off >> 2, r = off & 3;
  w[i] |= v << (8 * r);
  if (r != 0 && i + 1 < HW) w[i + 1] |= v >> (32 - 8 * r);
}
template <int HW>
RB_DG_HD void dg_put_u8(uint32_t (&w)[HW], int off, uint32_t v) {
  w[off >> 2] |= (v & 0xFFu) << (8 * (off & 3));
}
template <int HW>
RB_DG_HD void dg_put_u64(uint32_t (&w)[HW], int off, uint64_t v) {
  dg_put_u32(w, off, static_cast<uint32_t>(v));
  dg_put_u32(w, off + 4, static_cast<uint32_t>(v >> 32));
}

// bytes sh .. sh + 15 of the 32 bytes (a, b), sh in 0..15 known at compile time
RB_DG_HD DgChunk dg_extract16(const DgChunk& a, const DgChunk& b, int sh) {
  const uint32_t win[9] = {a.w[0], a.w[1], a.w[2], a.w[3], b.w[0], b.w[1], b.w[2], b.w[3], 0u};
  const int q = sh >> 2, r = sh & 3;
  DgChunk o;
  RB_DG_UNROLL
  for (int i = 0; i < 4; ++i) o.w[i] = dg_funnel(win[q + i], win[q + i + 1], r);
  return o;
}

// ---------------------------------------------------------------------------------------------
// Parse

struct DgEndpoint {  // what one parse call gathers for one endpoint
  int32_t acked, frame_advantage, rtt_ms;  // in/out
  uint32_t received, disconnect_requested, reply_owed, status;
  uint64_t ping_lo, ping_hi;                // the u128 of the last QualityReport
  int32_t peer_last[4];                     // merged over this call's Inputs, from NULL_FRAME
  uint32_t peer_disconnected;               // bit i: player i, from 0
  int32_t input_slot, payload_len, start_frame;  // the last Input in slot order (slot -1: none)
  uint32_t report_slots;                    // bit m: slot m holds an accepted ChecksumReport
};

RB_DG_HD DgEndpoint dg_endpoint(int32_t acked, int32_t frame_advantage, int32_t rtt_ms) {
  DgEndpoint e{};
  e.acked = acked;
  e.frame_advantage = frame_advantage;
  e.rtt_ms = rtt_ms;
  RB_DG_UNROLL
  for (int i = 0; i < 4; ++i) e.peer_last[i] = kDgNullFrame;
  e.input_slot = -1;
  return e;
}

// One datagram of `avail` = min(dg_length, stride) > 0 bytes whose first 4 * kHeadWords bytes are in w
// (bytes at or above avail hold anything: no decision reads them).  bincode::deserialize first, and a
// datagram it refuses is dropped by the socket (udp_socket.rs:42); then handle_message.
template <int P>
RB_DG_HD void dg_parse_one(const uint32_t (&w)[DgLayout<P>::kHeadWords], int32_t avail, int slot, uint32_t remote_magic,
                           int64_t now_ms, DgEndpoint& e) {
  using Y = DgLayout<P>;
  constexpr int HW = Y::kHeadWords;
  if (avail < kDgHeaderBytes) {
    e.status |= kDgMalformed;
    return;
  }
  const uint32_t magic = w[0] & 0xFFFFu, variant = dg_u32<HW>(w, 2);
  bool ok = variant <= kDgKeepAlive;
  int32_t payload_len = 0;
  if (variant == kDgInput) {
    ok = avail >= Y::kPayload;  // the fixed part, whatever field the datagram stops in
    if (ok) {
      ok = dg_u64<HW>(w, Y::kCount) == static_cast<uint64_t>(P);  // a stated deviation: the reference indexes out of bounds
      uint32_t bools = dg_u8<HW>(w, Y::kRequested);
      RB_DG_UNROLL
      for (int i = 0; i < P; ++i) bools |= dg_u8<HW>(w, Y::kStatus + 5 * i);
      ok = ok && bools <= 1u;
      // the length as 64 bits, against the bytes left, before it forms any address
      const uint64_t len = dg_u64<HW>(w, Y::kLen);
      ok = ok && len <= static_cast<uint64_t>(avail - Y::kPayload);
      payload_len = static_cast<int32_t>(len);
    }
  } else {
    const int need = variant == kDgQualityReport ? 17 : variant == kDgQualityReply ? 16 : variant == kDgChecksumReport ? 20
                     : variant == kDgKeepAlive ? 0 : 4;
    ok = ok && avail >= kDgHeaderBytes + need;
  }
  if (!ok) {
    e.status |= kDgMalformed;
    return;
  }
  if (remote_magic != 0u && magic != remote_magic) {  // protocol.rs:551
    e.status |= kDgMagicMismatch;
    return;
  }
  e.received = 1u;  // protocol.rs:555-556
  if (variant == kDgInput) {  // on_input, protocol.rs:616-637
    const int32_t ack = static_cast<int32_t>(dg_u32<HW>(w, Y::kAck));
    e.acked = ack > e.acked ? ack : e.acked;  // pop_pending_output is monotone
    if (dg_u8<HW>(w, Y::kRequested)) {
      e.disconnect_requested = 1u;
    } else {
      RB_DG_UNROLL
      for (int i = 0; i < P; ++i) {
        const int32_t lf = static_cast<int32_t>(dg_u32<HW>(w, Y::kStatus + 5 * i + 1));
        e.peer_last[i] = lf > e.peer_last[i] ? lf : e.peer_last[i];
        e.peer_disconnected |= dg_u8<HW>(w, Y::kStatus + 5 * i) << i;
      }
    }
    e.input_slot = slot;
    e.payload_len = payload_len;
    e.start_frame = static_cast<int32_t>(dg_u32<HW>(w, Y::kStart));
  } else if (variant == kDgInputAck) {  // on_input_ack
    const int32_t ack = static_cast<int32_t>(dg_u32<HW>(w, kDgHeaderBytes));
    e.acked = ack > e.acked ? ack : e.acked;
  } else if (variant == kDgQualityReport) {  // on_quality_report, protocol.rs:697-701
    e.frame_advantage = static_cast<int32_t>(static_cast<int8_t>(dg_u8<HW>(w, kDgHeaderBytes)));
    e.reply_owed = 1u;
    e.ping_lo = dg_u64<HW>(w, kDgHeaderBytes + 1);
    e.ping_hi = dg_u64<HW>(w, kDgHeaderBytes + 9);
  } else if (variant == kDgQualityReply) {  // on_quality_reply, protocol.rs:704-708
    const uint64_t lo = dg_u64<HW>(w, kDgHeaderBytes), hi = dg_u64<HW>(w, kDgHeaderBytes + 8);
    const uint64_t now = static_cast<uint64_t>(now_ms);
    if (hi != 0u || lo > now || now - lo > 0x7FFFFFFFu) e.status |= kDgBadPong;  // the reference asserts millis >= pong
    else e.rtt_ms = static_cast<int32_t>(now - lo);
  } else if (variant == kDgChecksumReport) {
    e.report_slots |= 1u << slot;
  } else if (variant != kDgKeepAlive) {  // SyncRequest / SyncReply: the handshake is the caller's
    e.status |= kDgSyncSeen;
  }
}

struct DgReport {  // rb_checksum_report's fields
  uint64_t lo, hi;
  int32_t frame;
};
template <int HW>
RB_DG_HD DgReport dg_report_of(const uint32_t (&w)[HW]) {
  return DgReport{dg_u64<HW>(w, kDgHeaderBytes), dg_u64<HW>(w, kDgHeaderBytes + 8),
                  static_cast<int32_t>(dg_u32<HW>(w, kDgHeaderBytes + 16))};
}

// Appending `fresh` reports to the `kept` an endpoint holds: the oldest `drop` of the kept + fresh
// leave, the rest end up in entries 0 .. count - 1.
struct DgReportPlan {
  int32_t kept, drop, count;
};
RB_DG_HD DgReportPlan dg_report_plan(int32_t count_in, int fresh) {
  DgReportPlan p;
  p.kept = count_in < 0 ? 0 : count_in > kDgReportsKept ? kDgReportsKept : count_in;
  const int total = p.kept + fresh;
  p.drop = total > kDgReportsKept ? total - kDgReportsKept : 0;
  p.count = total - p.drop;
  return p;
}

RB_DG_HD int dg_popcount8(uint32_t x) {
  int n = 0;
  RB_DG_UNROLL
  for (int i = 0; i < kDgMaxSlots; ++i) n += static_cast<int>((x >> i) & 1u);
  return n;
}

// The copy of `n` bytes that start at byte `off` (known at compile time) of a source read in
// aligned 16-byte chunks, load(c) for c < src_chunks (others count as zero), to 16-byte chunks
// store(c, chunk), c < ceil(n / 16), through a two-chunk window.  The bytes of the last chunk past n
// are the source's next bytes or zero.
template <int kOff, class Load, class Store>
RB_DG_HD void dg_copy_from(Load load, int32_t src_chunks, int32_t n, Store store) {
  constexpr int a0 = kOff >> 4, sh = kOff & 15;
  const DgChunk zero{{0u, 0u, 0u, 0u}};
  const int32_t out_chunks = (n + 15) >> 4;
  DgChunk lo = a0 < src_chunks ? load(a0) : zero;
  DgChunk hi = (sh != 0 && a0 + 1 < src_chunks) ? load(a0 + 1) : zero;
  for (int32_t c = 0; c < out_chunks; ++c) {
    // the chunk after next is on its way before this one is stored
    const int32_t nx = a0 + c + (sh != 0 ? 2 : 1);
    const DgChunk next = (c + 1 < out_chunks && nx < src_chunks) ? load(nx) : zero;
    store(c, sh != 0 ? dg_extract16(lo, hi, sh) : lo);
    if (sh != 0) {
      lo = hi;
      hi = next;
    } else {
      lo = next;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Build

struct DgFixed {  // a message without a Vec: at most 26 bytes
  uint32_t w[8];
  int32_t len;
};

RB_DG_HD DgFixed dg_fixed(uint32_t magic, uint32_t variant) {
  DgFixed m{};
  m.w[0] = (magic & 0xFFFFu) | (variant << 16);  // the variant's upper bytes are zero
  m.len = kDgHeaderBytes;
  return m;
}
RB_DG_HD DgFixed dg_input_ack(uint32_t magic, int32_t ack_frame) {  // protocol.rs:495-501
  DgFixed m = dg_fixed(magic, kDgInputAck);
  dg_put_u32<8>(m.w, kDgHeaderBytes, static_cast<uint32_t>(ack_frame));
  m.len += 4;
  return m;
}
RB_DG_HD DgFixed dg_quality_reply(uint32_t magic, uint64_t pong_lo, uint64_t pong_hi) {  // protocol.rs:699-700
  DgFixed m = dg_fixed(magic, kDgQualityReply);
  dg_put_u64<8>(m.w, kDgHeaderBytes, pong_lo);
  dg_put_u64<8>(m.w, kDgHeaderBytes + 8, pong_hi);
  m.len += 16;
  return m;
}
RB_DG_HD DgFixed dg_quality_report(uint32_t magic, int32_t frame_advantage, int64_t now_ms) {  // protocol.rs:516-525
  DgFixed m = dg_fixed(magic, kDgQualityReport);
  dg_put_u8<8>(m.w, kDgHeaderBytes, static_cast<uint32_t>(frame_advantage));
  dg_put_u64<8>(m.w, kDgHeaderBytes + 1, static_cast<uint64_t>(now_ms));
  m.len += 17;
  return m;
}
RB_DG_HD DgFixed dg_checksum_report(uint32_t magic, const DgReport& r) {  // protocol.rs:736-742
  DgFixed m = dg_fixed(magic, kDgChecksumReport);
  dg_put_u64<8>(m.w, kDgHeaderBytes, r.lo);
  dg_put_u64<8>(m.w, kDgHeaderBytes + 8, r.hi);
  dg_put_u32<8>(m.w, kDgHeaderBytes + 16, static_cast<uint32_t>(r.frame));
  m.len += 20;
  return m;
}

struct DgOwed {  // what one endpoint owes this poll
  uint32_t magic;
  int64_t now_ms;
  int32_t input_len, start_frame, ack_frame;  // input_len <= 0: no Input
  uint32_t disconnect_requested;
  int32_t status_last[4];
  uint32_t status_disconnected;  // bit i: player i
  uint32_t ack_owed, reply_owed, report_due, keepalive_due;
  uint64_t ping_lo, ping_hi;
  int32_t frame_advantage;
  DgReport reports[kDgReportsKept];  // frame NULL_FRAME: none
};

// Input's fixed part, bytes 0 .. 30 + 5 P (protocol.rs:468-492)
template <int P>
RB_DG_HD void dg_input_head(const DgOwed& o, uint32_t (&w)[16]) {
  using Y = DgLayout<P>;
  RB_DG_UNROLL
  for (int i = 0; i < 16; ++i) w[i] = 0u;
  w[0] = (o.magic & 0xFFFFu) | (kDgInput << 16);
  dg_put_u32<16>(w, Y::kCount, static_cast<uint32_t>(P));
  RB_DG_UNROLL
  for (int i = 0; i < P; ++i) {
    dg_put_u8<16>(w, Y::kStatus + 5 * i, (o.status_disconnected >> i) & 1u);
    dg_put_u32<16>(w, Y::kStatus + 5 * i + 1, static_cast<uint32_t>(o.status_last[i]));
  }
  dg_put_u8<16>(w, Y::kRequested, o.disconnect_requested ? 1u : 0u);
  dg_put_u32<16>(w, Y::kStart, static_cast<uint32_t>(o.start_frame));
  dg_put_u32<16>(w, Y::kAck, static_cast<uint32_t>(o.ack_frame));
  dg_put_u32<16>(w, Y::kLen, static_cast<uint32_t>(o.input_len));
}

// The Input datagram: the head, then the packet's bytes from byte 31 + 5 P on.  load(c): 16-byte
// chunk c of the packet row, c < ceil(input_len / 16); store(c, chunk): chunk c of the datagram.
template <int P, class Load, class Store>
RB_DG_HD void dg_emit_input(const DgOwed& o, Load load, Store store) {
  constexpr int kOff = DgLayout<P>::kPayload, q = kOff >> 4, r = kOff & 15;
  uint32_t head[16];
  dg_input_head<P>(o, head);
  RB_DG_UNROLL
  for (int c = 0; c < q; ++c) store(c, DgChunk{{head[4 * c], head[4 * c + 1], head[4 * c + 2], head[4 * c + 3]}});
  // datagram chunk q + c holds packet bytes 16 c - r .. 16 c - r + 15: a copy that starts r bytes
  // before the packet, in a zero chunk, merged with the head's last bytes
  const int32_t src_chunks = (o.input_len + 15) >> 4;
  auto shifted = [&](int32_t c) -> DgChunk { return c == 0 ? DgChunk{{0u, 0u, 0u, 0u}} : load(c - 1); };
  dg_copy_from<r == 0 ? 16 : 16 - r>(shifted, src_chunks + 1, o.input_len + r, [&](int32_t c, DgChunk x) {
    if (c == 0)
      RB_DG_UNROLL
      for (int i = 0; i < 4; ++i) x.w[i] |= head[4 * q + i];
    store(q + c, x);
  });
}

// The messages in priority order, packed densely: emit_input(slot) / emit_fixed(slot, message) for
// each that fits the slots and the stride, length(slot, bytes) for its length.  Returns the count;
// status gets kDgNoRoom / kDgAdvantageRange for what was left out.
template <int P, class EmitInput, class EmitFixed>
RB_DG_HD int32_t dg_build_endpoint(const DgOwed& o, int32_t slots, int64_t stride, uint32_t& status, EmitInput emit_input,
                                   EmitFixed emit_fixed) {
  int32_t count = 0;
  auto room = [&](int64_t bytes) -> bool {
    if (count < slots && bytes <= stride) return true;
    status |= kDgNoRoom;
    return false;
  };
  if (o.input_len > 0 && room(static_cast<int64_t>(DgLayout<P>::kPayload) + o.input_len))
    emit_input(count++, DgLayout<P>::kPayload + o.input_len);
  if (o.ack_owed && room(10)) emit_fixed(count++, dg_input_ack(o.magic, o.ack_frame));
  if (o.reply_owed && room(22)) emit_fixed(count++, dg_quality_reply(o.magic, o.ping_lo, o.ping_hi));
  if (o.report_due) {
    if (o.frame_advantage < -128 || o.frame_advantage > 127) status |= kDgAdvantageRange;  // the reference panics, :519-520
    else if (room(23)) emit_fixed(count++, dg_quality_report(o.magic, o.frame_advantage, o.now_ms));
  }
  RB_DG_UNROLL
  for (int k = 0; k < kDgReportsKept; ++k)
    if (o.reports[k].frame != kDgNullFrame && room(26)) emit_fixed(count++, dg_checksum_report(o.magic, o.reports[k]));
  if (o.keepalive_due && count == 0 && room(kDgHeaderBytes)) emit_fixed(count++, dg_fixed(o.magic, kDgKeepAlive));
  return count;
}

}  // namespace rb
