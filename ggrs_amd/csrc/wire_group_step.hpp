// ggrs_amd/csrc/wire_group_step.hpp — one endpoint's share of rb_decode_input_packets_grouped and
// rb_encode_input_packets_grouped (include/ggrs_amd.h): UdpProtocol::on_input
// (network/protocol.rs:616-689) and send_pending_output (:468-493) for an endpoint that carries a
// group of K handles in one stream.  A frame of the stream is the members' inputs one after the
// other, ascending by handle (InputBytes::from_inputs, :61-79; to_player_inputs, :81-93): K * IB
// bytes, 1 to 16.
// Plain C++, no device include: the kernels (wire_group.hip) and the host check
// (tests/check_wire_group.cpp) call the same functions; memory is reached through the caller's Io
// only, so each side brings its own layout and its own bounds.
//
// A frame lives in (K * IB + 3) / 4 words, byte 0 in the low byte of word 0.  The stream is walked
// a byte at a time by shifting whole frames: the reference rotates (its low byte leaves and comes
// back in at the top), the frame being decoded fills from the top.  Every word index is a constant.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RB_WG_HD __host__ __device__ __forceinline__
#define RB_WG_UNROLL _Pragma("unroll")
#define RB_WG_NOUNROLL _Pragma("nounroll")
#else
#define RB_WG_HD inline __attribute__((always_inline))
#define RB_WG_UNROLL
#define RB_WG_NOUNROLL
#endif

namespace rb {

constexpr int32_t kWgNull = -1;
constexpr int32_t kWgOk = 0, kWgNothing = 1, kWgMalformed = -1, kWgGap = -2;  // decode status
constexpr int32_t kWgEncNothing = 0, kWgEncTooLong = -1, kWgEncOverrun = -2;  // encode lengths
constexpr uint32_t kWgRunMin = 4;  // the shortest run of 0x00 / 0xFF the encoder compresses

// bytes r .. r + 3 of the eight bytes (lo, hi), r in 0..3
RB_WG_HD uint32_t wg_funnel(uint32_t lo, uint32_t hi, uint32_t r) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, r);
#else
  return r == 0 ? lo : (lo >> (8 * r)) | (hi << (32 - 8 * r));
#endif
}

// drop the first byte of N words
template <int N>
RB_WG_HD void wg_shift(uint32_t (&w)[N]) {
  RB_WG_UNROLL
  for (int i = 0; i < N - 1; ++i) w[i] = wg_funnel(w[i], w[i + 1], 1);
  w[N - 1] >>= 8;
}

template <int IB, int K>
struct WgFrame {
  static_assert((IB == 1 || IB == 2 || IB == 4) && K >= 1 && K <= 4, "inputs of 1, 2 or 4 bytes, one to four members");
  static constexpr int kBytes = IB * K;
  static constexpr int kWords = (kBytes + 3) / 4;
};

// drop a frame's first byte and bring b in as its last
template <int FB, int N>
RB_WG_HD void wg_push(uint32_t (&w)[N], uint32_t b) {
  wg_shift(w);
  w[(FB - 1) >> 2] |= b << (8 * ((FB - 1) & 3));
}

// member m's input of a frame (m a constant at every call)
template <int IB, int N>
RB_WG_HD uint32_t wg_member(const uint32_t (&w)[N], int m) {
  if (IB == 4) return w[m];
  if (IB == 2) return (w[m >> 1] >> (16 * (m & 1))) & 0xFFFFu;
  return (w[0] >> (8 * m)) & 0xFFu;
}
template <int IB, int N>
RB_WG_HD void wg_set_member(uint32_t (&w)[N], int m, uint32_t v) {
  w[(m * IB) >> 2] |= v << (8 * ((m * IB) & 3));
}

// The LEB128 header of a segment, by the rules of wire_varint.hpp (which is device code): up to
// ten bytes, a value that reaches 2^32 is malformed, padded groups past the fifth byte are not.
template <class Next>
RB_WG_HD bool wg_varint_get(const int32_t& pos, int32_t n, Next&& next, uint32_t& hdr) {
  hdr = 0;
  bool big = false;
  for (int i = 0; i < 10; ++i) {
    if (pos >= n) return false;
    const uint32_t b = next();
    const uint32_t v = b & 0x7Fu;
    if (i < 4) hdr |= v << (7 * i);
    else if (i == 4) {
      hdr |= v << 28;
      big |= (v >> 4) != 0;
    } else if (i < 9) big |= v != 0;
    else big |= (v & 1u) != 0;
    if (!(b & 0x80u)) return !big;
  }
  return false;
}

// ---------------------------------------------------------------------------------------------
// Decode.  Io: uint32_t load(int m, size_t slot), void store(int m, size_t slot, uint32_t v) on
// member m's column of the inputs tensor (slot: the ring slot or the frame), and
// void chunk(int32_t off, uint32_t (&w)[4]): bytes off .. off + 15 of the packet, off a multiple
// of 16 below n (bytes at and past n may hold anything).
// n, start, last: the lead row's length, start frame and watermark; head: the packet's first 32
// bytes.  Returns the status; `decoded` says that the packet was taken (every member's watermark
// row is then `newest`, which may equal `last`).
template <int IB, int K, bool kRing, class Io>
RB_WG_HD int32_t wg_decode(Io& io, int32_t n, int32_t start, int32_t last, const uint32_t (&head)[8], int64_t packet_stride,
                           int32_t frames, int32_t max_prediction, int32_t& newest, bool& decoded) {
  constexpr int FB = WgFrame<IB, K>::kBytes, FW = WgFrame<IB, K>::kWords;
  const uint32_t rmask = static_cast<uint32_t>(frames) - 1u;  // kRing: frames is the ring's power of two
  const int64_t rf = static_cast<int64_t>(start) - 1;          // the reference input's frame
  // every member's reference input before the checks: the ring has every slot, the linear index is
  // clamped and the value dropped below when the checks say there is no reference
  const size_t rslot = kRing ? (static_cast<uint32_t>(rf) & rmask)
                             : static_cast<size_t>(rf < 0 ? 0 : rf >= frames ? frames - 1 : rf);
  uint32_t ref[FW];
  RB_WG_UNROLL
  for (int i = 0; i < FW; ++i) ref[i] = 0;
  RB_WG_UNROLL
  for (int m = 0; m < K; ++m) wg_set_member<IB>(ref, m, io.load(m, rslot));
  newest = last;
  decoded = false;
  if (n <= 0) return kWgNothing;               // no packet from this endpoint
  if (n > packet_stride) return kWgMalformed;  // the row does not hold that many bytes
  if (last != kWgNull) {
    if (static_cast<int64_t>(last) + 1 < start) return kWgGap;  // protocol.rs:639-642
    // protocol.rs:646-653: a reference older than recv_inputs keeps, or below NULL_FRAME: ignored
    if (rf < static_cast<int64_t>(last) - 2 * static_cast<int64_t>(max_prediction) || rf < kWgNull) return kWgNothing;
  }
  if (!kRing && rf >= frames) return kWgMalformed;  // the reference lies past the caller's tensor
  if (last == kWgNull || rf == kWgNull) {           // recv_inputs[NULL_FRAME] is the zeroed input
    RB_WG_UNROLL
    for (int i = 0; i < FW; ++i) ref[i] = 0;
  }
  // the frames this call may write: above `last` (protocol.rs:661-663), never below 0, and below
  // `frames` (linear) or the first R of them (ring: no slot twice)
  const int64_t wlo = last < 0 ? 0 : static_cast<int64_t>(last) + 1;
  const int64_t whi = kRing ? (start > wlo ? start : wlo) + rmask : static_cast<int64_t>(frames) - 1;
  // One literal of every byte within the 32-byte head, or one run: valid by the header alone, so
  // the validating pass is skipped.  Every other packet: pass 0 validates without a store (a
  // malformed packet leaves the tensor as it was, protocol.rs:656), pass 1 writes.
  const uint32_t h0 = head[0] & 0xFFu;
  const bool lit = !(h0 & 0x81u) && static_cast<int32_t>(h0 >> 1) == n - 1 && n <= 32 && (n - 1) % FB == 0;
  const bool run = (h0 & 0x81u) == 1u && n == 1 && (h0 >> 2) % FB == 0;
  for (int pass = (lit || run) ? 1 : 0; pass < 2; ++pass) {
    uint32_t win[8], cur[FW];
    RB_WG_UNROLL
    for (int i = 0; i < 8; ++i) win[i] = head[i];
    RB_WG_UNROLL
    for (int i = 0; i < FW; ++i) cur[i] = 0;
    int32_t pos = 0;
    uint32_t at = 0;  // bytes of the current frame so far (pass 0: the stream's length modulo FB)
    int64_t f = start;
    bool ok = true, past = false;
    // the window holds bytes pos .. pos + 31 - (pos & 15); its upper half is refilled, one aligned
    // 16-byte chunk at a time, whenever the lower half has been used up
    auto next = [&]() __attribute__((always_inline)) -> uint32_t {
      const uint32_t b = win[0] & 0xFFu;
      wg_shift(win);
      ++pos;
      if ((pos & 15) == 0 && pos + 16 < n) {
        uint32_t c[4];
        io.chunk(pos + 16, c);
        RB_WG_UNROLL
        for (int i = 0; i < 4; ++i) win[4 + i] = c[i];
      }
      return b;
    };
    auto emit = [&](uint32_t x) __attribute__((always_inline)) {  // pass 1: one byte of the XOR stream
      const uint32_t r = ref[0] & 0xFFu;
      wg_push<FB>(ref, r);
      wg_push<FB>(cur, r ^ x);
      if (++at == static_cast<uint32_t>(FB)) {
        at = 0;
        if (f >= wlo && f <= whi) {
          const size_t slot = kRing ? (static_cast<uint32_t>(f) & rmask) : static_cast<size_t>(f);
          RB_WG_UNROLL
          for (int m = 0; m < K; ++m) io.store(m, slot, wg_member<IB>(cur, m));
          newest = static_cast<int32_t>(f);
        }
        past = f >= whi;  // nothing after this frame is written: the rest of the packet is validated already
        ++f;
      }
    };
    while (pos < n && !past) {
      uint32_t hdr;
      if (!wg_varint_get(pos, n, next, hdr)) {
        ok = false;
        break;
      }
      if (hdr & 1u) {  // a run of 0x00 / 0xFF bytes
        const uint32_t len = hdr >> 2;
        if (len > (1u << 16)) {
          ok = false;
          break;
        }
        if (pass == 0) {
          at = (at + len) % FB;
        } else {
          const uint32_t x = (hdr & 2u) ? 0xFFu : 0u;
          for (uint32_t i = 0; i < len && !past; ++i) emit(x);
        }
      } else {  // literal bytes
        const uint32_t len = hdr >> 1;
        if (len > static_cast<uint32_t>(n - pos)) {
          ok = false;
          break;
        }
        if (pass == 0) at = (at + len) % FB;
        for (uint32_t i = 0; i < len && !past; ++i) {
          const uint32_t x = next();
          if (pass == 1) emit(x);
        }
      }
    }
    // compression.rs:47 and to_player_inputs (protocol.rs:81-93): whole frames of the group only
    if (pass == 0 && (!ok || at != 0)) return kWgMalformed;
  }
  decoded = true;
  return newest == last ? kWgNothing : kWgOk;
}

// ---------------------------------------------------------------------------------------------
// Encode.  Io: uint32_t load(int m, size_t slot) on member m's column of the sender's inputs,
// void store_byte(int32_t pos, uint32_t b) for packet bytes from the 33rd on, and
// void store16(int i, const uint32_t (&w)[4]) for bytes 16 i .. 16 i + 15 of the row, i in 0..1.
// acked, newest: the lead row's.  Returns the length code; `start` is the packet's start frame
// (written by the caller whatever the code).
template <int IB, int K, bool kRing, class Io>
RB_WG_HD int32_t wg_encode(Io& io, int32_t acked, int32_t newest, int32_t first_frame, int32_t frames, int64_t cap,
                           int32_t& start_out) {
  constexpr int FB = WgFrame<IB, K>::kBytes, FW = WgFrame<IB, K>::kWords;
  constexpr int kAhead = K == 1 ? 4 : 2;  // frames loaded ahead of the scan
  const uint32_t rmask = static_cast<uint32_t>(frames) - 1u;
  // pending_output starts after the last ack, or at the sender's first input before any ack
  // (protocol.rs:471-476)
  const int64_t start = acked == kWgNull ? first_frame : static_cast<int64_t>(acked) + 1;
  start_out = static_cast<int32_t>(start);
  if (newest < start || start < 0 || (!kRing && newest >= frames)) return kWgEncNothing;
  // from here 0 <= start <= newest, and acked is NULL_FRAME or start - 1 >= 0
  const uint32_t count = static_cast<uint32_t>(newest - start) + 1u;  // frames to send
  if (kRing && count + (acked != kWgNull ? 1u : 0u) > rmask + 1u) return kWgEncOverrun;  // the reference's slot is gone
  auto load_slot = [&](size_t slot, uint32_t (&w)[FW]) __attribute__((always_inline)) {
    RB_WG_UNROLL
    for (int i = 0; i < FW; ++i) w[i] = 0;
    RB_WG_UNROLL
    for (int m = 0; m < K; ++m) wg_set_member<IB>(w, m, io.load(m, slot));
  };
  auto load_frame = [&](uint32_t i, uint32_t (&w)[FW]) __attribute__((always_inline)) {  // frame i of the packet, i < count
    const int64_t f = start + i;
    load_slot(kRing ? (static_cast<uint32_t>(f) & rmask) : static_cast<size_t>(f), w);
  };
  // one round trip: the reference and the first frames (indices clamped to the packet's last)
  uint32_t ref[FW], pre[kAhead][FW];
  load_slot(kRing ? (static_cast<uint32_t>(acked) & rmask) : static_cast<size_t>(acked < 0 ? 0 : acked), ref);
  RB_WG_UNROLL
  for (int a = 0; a < kAhead; ++a) load_frame(static_cast<uint32_t>(a) < count ? a : count - 1, pre[a]);
  if (acked == kWgNull) {
    RB_WG_UNROLL
    for (int i = 0; i < FW; ++i) ref[i] = 0;
  }

  uint32_t win[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // the packet's first 32 bytes, shifted in from the top
  int32_t pos = 0;
  bool ok = true;
  auto put = [&](uint32_t b) __attribute__((always_inline)) {
    if (pos >= cap) {
      ok = false;
      return;
    }
    if (pos < 32) {
      wg_shift(win);
      win[7] |= b << 24;
    } else {
      io.store_byte(pos, b);
    }
    ++pos;
  };
  auto put_header = [&](uint32_t v) __attribute__((always_inline)) {  // LEB128
    while (v >= 0x80u) {
      put((v & 0x7Fu) | 0x80u);
      v >>= 7;
    }
    put(v);
  };
  // bytes a .. b - 1 of the XOR stream as one literal segment, read again from the cache the scan filled
  auto flush = [&](uint32_t a, uint32_t b) __attribute__((always_inline)) {
    if (b <= a) return;
    put_header((b - a) << 1);
    uint32_t fi = a / FB, j = a % FB, w[FW];
    load_frame(fi, w);
    RB_WG_UNROLL
    for (int i = 0; i < FW; ++i) w[i] ^= ref[i];
    for (uint32_t t = 0; t < j; ++t) wg_shift(w);
    for (uint32_t i = a; i < b && ok; ++i) {
      put(w[0] & 0xFFu);
      wg_shift(w);
      if (++j == static_cast<uint32_t>(FB) && i + 1 < b) {
        j = 0;
        load_frame(++fi, w);
        RB_WG_UNROLL
        for (int q = 0; q < FW; ++q) w[q] ^= ref[q];
      }
    }
  };
  // One scan over the stream's bytes: a maximal run of >= kWgRunMin equal 0x00 / 0xFF bytes becomes
  // a compressed segment, everything between two of them one literal (the oracle's wire::rle_encode).
  // A run may end inside one member's input and the literal begin in the next: the stream knows
  // nothing of members.
  uint32_t lit = 0, run_at = 0, run_byte = 0x100u, k = 0;
  auto close_run = [&](uint32_t end) __attribute__((always_inline)) {
    if ((run_byte == 0u || run_byte == 0xFFu) && end - run_at >= kWgRunMin) {
      flush(lit, run_at);
      put_header(((end - run_at) << 2) | (run_byte ? 2u : 0u) | 1u);
      lit = end;
    }
  };
  for (uint32_t fi = 0; fi < count && ok; ++fi) {
    uint32_t x[FW];
    RB_WG_UNROLL
    for (int i = 0; i < FW; ++i) x[i] = pre[0][i] ^ ref[i];
    RB_WG_UNROLL
    for (int a = 0; a < kAhead - 1; ++a) {
      RB_WG_UNROLL
      for (int i = 0; i < FW; ++i) pre[a][i] = pre[a + 1][i];
    }
    load_frame(fi + kAhead < count ? fi + kAhead : count - 1, pre[kAhead - 1]);
    RB_WG_NOUNROLL
    for (int j = 0; j < FB && ok; ++j, ++k) {
      const uint32_t b = x[0] & 0xFFu;
      wg_shift(x);
      if (b != run_byte) {
        close_run(k);
        run_at = k;
        run_byte = b;
      }
    }
  }
  if (ok) close_run(k);
  if (ok) flush(lit, k);
  if (!ok) return kWgEncTooLong;  // the packet does not fit the row
  // bring byte 0 down to the window's first byte: (32 - pos) bytes to drop, pos >= 1
  if (pos < 32) {
    const uint32_t m = 32u - static_cast<uint32_t>(pos);
    if (m & 16u) {
      RB_WG_UNROLL
      for (int i = 0; i < 4; ++i) win[i] = win[i + 4], win[i + 4] = 0;
    }
    if (m & 8u) {
      RB_WG_UNROLL
      for (int i = 0; i < 8; ++i) win[i] = i + 2 < 8 ? win[i + 2] : 0u;
    }
    if (m & 4u) {
      RB_WG_UNROLL
      for (int i = 0; i < 8; ++i) win[i] = i + 1 < 8 ? win[i + 1] : 0u;
    }
    const uint32_t r = m & 3u;
    RB_WG_UNROLL
    for (int i = 0; i < 7; ++i) win[i] = wg_funnel(win[i], win[i + 1], r);
    win[7] >>= 8 * r;
  }
  const uint32_t lo[4] = {win[0], win[1], win[2], win[3]}, hi[4] = {win[4], win[5], win[6], win[7]};
  io.store16(0, lo);
  if (pos > 16) io.store16(1, hi);
  return pos;
}

// Groups: byte g of group_masks is the handle mask of group g (0: none).  At least one group, no
// bit at or above num_players, no handle in two groups.
inline bool wg_groups_ok(uint32_t group_masks, int32_t num_players) {
  if (group_masks == 0 || num_players <= 0 || num_players > 4) return false;
  uint32_t seen = 0;
  for (int g = 0; g < 4; ++g) {
    const uint32_t m = (group_masks >> (8 * g)) & 0xFFu;
    if ((m >> num_players) != 0 || (m & seen) != 0) return false;
    seen |= m;
  }
  return true;
}

}  // namespace rb
