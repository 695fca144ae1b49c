// ggrs_amd/csrc/wire.hip — batched input packets: the
// encode of UdpProtocol::send_pending_output (protocol.rs:468-500) and the
// decode of UdpProtocol::on_input (protocol.rs:616-689) for one endpoint per
// (session, remote handle), straight into the P2P batch's delivery tensors.
//
// Wire format (network/compression.rs): XOR delta of every pending input
// against the reference input (the last acked one), then bitfield RLE
// (bitfield-rle 0.2): varint-headed sequences, odd header = a run of
// `header >> 2` bytes of 0x00 / 0xFF (bit 1), even header = `header >> 1`
// literal bytes.  Varints are unsigned LEB128.  The encoder compresses runs of
// >= 4 equal 0x00/0xFF bytes (the same rule as oracle/ggrs_oracle.hpp wire::).
//
// One lane per endpoint: packets are a few bytes (one input per frame since
// the last ack), so the work is a short serial parse per lane; lanes of a wave
// read consecutive packet rows and write consecutive sessions of one frame.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ggrs_amd.h"
#include "wire_varint.hpp"

namespace {

constexpr int32_t kNull = -1;
constexpr int kRunMin = 4;

// status codes per endpoint (rb_decode_input_packets)
constexpr int32_t kDecOk = 0, kDecNothing = 1, kDecMalformed = -1, kDecGap = -2;

struct DecParams {
  const uint8_t* packets;
  int64_t packet_stride;
  const int32_t* lengths;
  const int32_t* start_frames;
  uint8_t* remote_inputs;  // [remote_frames][P][S] Input values of input_bytes
  int32_t* remote_upto;    // [P][S]
  int32_t* status;         // [S]
  int32_t handle, P, S, IB, remote_frames, max_prediction;
};

__device__ __forceinline__ uint8_t in_byte(const uint8_t* base, int32_t f, int h, int P, int S, int s, int IB, int i) {
  return base[((static_cast<size_t>(f) * P + h) * S + s) * IB + i];
}

__global__ void __launch_bounds__(256) decode_packets_kernel(const DecParams p) {
  const int s = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= p.S) return;
  const int h = p.handle, IB = p.IB;
  int32_t* up = p.remote_upto + static_cast<size_t>(h) * p.S + s;
  const int32_t last = *up;
  const int32_t start = p.start_frames[s];
  const int32_t n = p.lengths[s];
  const uint8_t* d = p.packets + static_cast<int64_t>(s) * p.packet_stride;
  if (n <= 0) {  // no packet from this endpoint this tick
    p.status[s] = kDecNothing;
    return;
  }
  // a length past the row would read the next endpoint's packet (or past the tensor): the
  // datagram is not what the row holds, so it is malformed
  if (n > p.packet_stride) {
    p.status[s] = kDecMalformed;
    return;
  }
  // protocol.rs:639-642: a packet must not skip frames we never received
  if (last != kNull && last + 1 < start) {
    p.status[s] = kDecGap;
    return;
  }
  // protocol.rs:646-653: decode against the input before start_frame (blank
  // before the first input); recv_inputs keeps only the last 2*max_prediction
  // frames, so an older reference means the packet is ignored
  if (last != kNull && start - 1 < last - 2 * p.max_prediction) {
    p.status[s] = kDecNothing;
    return;
  }
  // recv_inputs never holds a frame below NULL_FRAME: such a packet finds no
  // decode input and is ignored (protocol.rs:653); a reference input past the
  // caller's remote_inputs tensor cannot be read at all
  if (last != kNull && start - 1 < kNull) {
    p.status[s] = kDecNothing;
    return;
  }
  if (start - 1 >= p.remote_frames) {
    p.status[s] = kDecMalformed;
    return;
  }
  uint8_t ref[4] = {0, 0, 0, 0};  // recv_inputs[NULL_FRAME] is the zeroed input (protocol.rs:213-214)
  if (last != kNull && start - 1 != kNull)
    for (int i = 0; i < IB; ++i) ref[i] = in_byte(p.remote_inputs, start - 1, h, p.P, p.S, s, IB, i);
  // bitfield RLE decode fused with delta decode: byte k of the XOR stream is
  // byte (k % IB) of input k / IB
  int32_t k = 0, newest = last;
  uint8_t cur[4] = {0, 0, 0, 0};
  auto emit = [&](uint8_t x) {
    const int i = k % IB;
    cur[i] = static_cast<uint8_t>(ref[i] ^ x);
    if (i == IB - 1) {
      const int32_t f = start + k / IB;
      if (f > last && f < p.remote_frames) {  // protocol.rs:661-663: skip inputs already received
        uint8_t* dst = p.remote_inputs + ((static_cast<size_t>(f) * p.P + h) * p.S + s) * IB;
        for (int j = 0; j < IB; ++j) dst[j] = cur[j];
        newest = f;
      }
    }
    ++k;
  };
  // pass 0 validates without writing, pass 1 writes: a malformed packet (the reference panics before
  // any input is added, protocol.rs:656) leaves remote_inputs as it found them
  bool ok = true;
  for (int pass = 0; pass < 2 && ok; ++pass) {
    int32_t pos = 0;
    uint32_t nbytes = 0;  // pass 0: the XOR stream's length (mod 2^32: only its remainder by IB is read)
    while (pos < n && ok) {
      uint32_t hdr;
      if (!rb_wire::varint_get(pos, n, [&]() -> uint32_t { return d[pos++]; }, hdr)) {  // LEB128
        ok = false;
        break;
      }
      if (hdr & 1u) {  // compressed run of 0x00 / 0xFF
        const uint32_t len = hdr >> 2;
        if (len > (1u << 16)) {
          ok = false;
          break;
        }
        const uint8_t x = (hdr & 2u) ? 0xFF : 0x00;
        if (pass == 0) nbytes += len;
        else
          for (uint32_t i = 0; i < len; ++i) emit(x);
      } else {  // literal bytes
        const uint32_t len = hdr >> 1;
        if (len > static_cast<uint32_t>(n - pos)) {
          ok = false;
          break;
        }
        if (pass == 0) {
          nbytes += len;
          pos += static_cast<int32_t>(len);
        } else {
          for (uint32_t i = 0; i < len; ++i) emit(d[pos++]);
        }
      }
    }
    if (pass == 0 && nbytes % static_cast<uint32_t>(IB) != 0) ok = false;  // compression.rs:47 assert: whole inputs only
  }
  if (!ok) {
    p.status[s] = kDecMalformed;  // the reference panics ("decoding failed", protocol.rs:656)
    return;
  }
  *up = newest;
  p.status[s] = newest == last ? kDecNothing : kDecOk;
}

struct EncParams {
  const uint8_t* inputs;  // [frames][P][S] Input values by frame (the sender's local inputs)
  int32_t frames;
  const int32_t* acked;   // [S] last frame the receiver acked (kNull: none)
  const int32_t* newest;  // [S] newest frame to send
  uint8_t* packets;
  int64_t packet_stride;
  int32_t* lengths;
  int32_t* start_frames;
  int32_t handle, P, S, IB, first_frame;
};

__device__ __forceinline__ void put_varint(uint8_t* out, int32_t cap, int32_t& pos, uint32_t v, bool& ok) {
  while (v >= 0x80) {
    if (pos >= cap) {
      ok = false;
      return;
    }
    out[pos++] = static_cast<uint8_t>(v | 0x80);
    v >>= 7;
  }
  if (pos >= cap) {
    ok = false;
    return;
  }
  out[pos++] = static_cast<uint8_t>(v);
}

// send_pending_output: pending inputs (acked, newest] XOR the last acked input
// (blank before any ack), bitfield-RLE encoded.
__global__ void __launch_bounds__(256) encode_packets_kernel(const EncParams p) {
  const int s = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= p.S) return;
  const int h = p.handle, IB = p.IB;
  const int32_t acked = p.acked[s], newest = p.newest[s];
  // pending_output starts after the last ack, or at the sender's first input
  // (its input delay) before any ack (protocol.rs:471-476)
  const int32_t start = acked == kNull ? p.first_frame : acked + 1;
  uint8_t* out = p.packets + static_cast<int64_t>(s) * p.packet_stride;
  const int32_t cap = static_cast<int32_t>(p.packet_stride);
  p.start_frames[s] = start;
  if (newest < start || newest >= p.frames || start < 0) {
    p.lengths[s] = 0;
    return;
  }
  uint8_t ref[4] = {0, 0, 0, 0};
  if (acked != kNull)
    for (int i = 0; i < IB; ++i) ref[i] = in_byte(p.inputs, acked, h, p.P, p.S, s, IB, i);
  const int32_t total = (newest - start + 1) * IB;  // XOR stream length
  auto xb = [&](int32_t k) -> uint8_t {
    return static_cast<uint8_t>(ref[k % IB] ^ in_byte(p.inputs, start + k / IB, h, p.P, p.S, s, IB, k % IB));
  };
  int32_t pos = 0, lit = 0, k = 0;
  bool ok = true;
  auto flush = [&](int32_t end) {
    if (end > lit) {
      put_varint(out, cap, pos, static_cast<uint32_t>(end - lit) << 1, ok);
      for (int32_t i = lit; i < end && ok; ++i) {
        if (pos >= cap) ok = false;
        else out[pos++] = xb(i);
      }
    }
  };
  while (k < total && ok) {
    const uint8_t b = xb(k);
    int32_t j = k;
    if (b == 0x00 || b == 0xFF)
      while (j < total && xb(j) == b) ++j;
    if (j - k >= kRunMin) {
      flush(k);
      put_varint(out, cap, pos, (static_cast<uint32_t>(j - k) << 2) | (b ? 2u : 0u) | 1u, ok);
      k = lit = j;
    } else {
      k = j > k ? j : k + 1;
    }
  }
  flush(total);
  p.lengths[s] = ok ? pos : -1;  // -1: the packet does not fit packet_stride
}

// ---------------------------------------------------------------------------------------------
// The ring-native codec (rb_decode_input_packets_all / rb_encode_input_packets_all): every
// endpoint of a batch in one launch, into / out of a linear [frames][P][S] tensor or a delivery
// ring [R][P][S] (frame f in slot f & (R - 1)).  One lane per endpoint,
// handle-major: blockIdx.y walks the handles of the mask, so a wave holds 64 consecutive sessions
// of one handle and its loads and stores of one frame are one row of the tensor.
//
// Frame arithmetic is 64-bit and every tensor index is either masked (ring) or range-checked
// (linear) right where it is formed: addresses stay inside the tensors whatever the lengths,
// start frames and watermarks hold.

template <int IB> struct InputWord;
template <> struct InputWord<1> { using type = uint8_t; };
template <> struct InputWord<2> { using type = uint16_t; };
template <> struct InputWord<4> { using type = uint32_t; };

// the handles of a mask, one per byte, lowest first
__host__ inline uint32_t pack_handles(uint32_t mask, int& count) {
  uint32_t packed = 0;
  count = 0;
  for (uint32_t h = 0; h < 4; ++h)
    if ((mask >> h) & 1u) packed |= h << (8 * count++);
  return packed;
}

// a 32-byte window in 8 words, byte 0 in the low byte of w[0]: drop its first byte
__device__ __forceinline__ void window_shift(uint32_t (&w)[8]) {
#pragma unroll
  for (int i = 0; i < 7; ++i) w[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], 1);
  w[7] >>= 8;
}

struct DecAllParams {
  const uint8_t* packets;  // [P][S] rows of packet_stride bytes
  int64_t packet_stride;
  const int32_t* lengths;       // [P][S]
  const int32_t* start_frames;  // [P][S]
  uint8_t* inputs;              // [frames][P][S] Input values of IB bytes
  int32_t* upto;                // [P][S]
  int32_t* status;              // [P][S]
  int32_t P, S, frames, max_prediction;
  uint32_t handles;  // pack_handles
};

// UdpProtocol::on_input for the endpoint of handle h, session s
template <int IB, bool kRing>
__device__ __forceinline__ void decode_endpoint(const DecAllParams& p, int h, int s) {
  using T = typename InputWord<IB>::type;
  const size_t e = static_cast<size_t>(h) * p.S + s;
  const uint32_t rmask = static_cast<uint32_t>(p.frames) - 1u;  // kRing: frames is the ring's power of two
  T* const col = reinterpret_cast<T*>(p.inputs) + e;            // frame / slot 0 of this endpoint
  const size_t plane = static_cast<size_t>(p.P) * p.S;
  // every load whose address the lane knows: head words first, then the reference input
  int32_t n = p.lengths[e], start = p.start_frames[e], last = p.upto[e];
  const uint8_t* pk = p.packets + static_cast<int64_t>(e) * p.packet_stride;
  uint4 head0 = reinterpret_cast<const uint4*>(pk)[0], head1 = reinterpret_cast<const uint4*>(pk)[1];
#if defined(__HIP_DEVICE_COMPILE__)
  // all five loads are in flight before the first is waited for: without this the compiler sinks
  // the others below the `n <= 0` branch, a round trip of their own
  asm volatile("" : "+v"(n), "+v"(start), "+v"(last), "+v"(head0.x), "+v"(head0.y), "+v"(head0.z), "+v"(head0.w),
               "+v"(head1.x), "+v"(head1.y), "+v"(head1.z), "+v"(head1.w));
#endif
  const int64_t rf = static_cast<int64_t>(start) - 1;  // the reference input's frame
  // (loaded before the checks: the ring has every slot, the linear index is clamped and the value
  // dropped below when the checks say there is no reference)
  const size_t rslot = kRing ? (static_cast<uint32_t>(rf) & rmask)
                             : static_cast<size_t>(rf < 0 ? 0 : rf >= p.frames ? p.frames - 1 : rf);
  uint32_t ref = col[rslot * plane];
  int32_t* const st = p.status + e;
  if (n <= 0) {  // no packet from this endpoint
    *st = kDecNothing;
    return;
  }
  if (n > p.packet_stride) {  // the row does not hold that many bytes
    *st = kDecMalformed;
    return;
  }
  if (last != kNull) {
    if (static_cast<int64_t>(last) + 1 < start) {  // protocol.rs:639-642
      *st = kDecGap;
      return;
    }
    // protocol.rs:646-653: a reference older than recv_inputs keeps, or below NULL_FRAME: ignored
    if (rf < static_cast<int64_t>(last) - 2 * static_cast<int64_t>(p.max_prediction) || rf < kNull) {
      *st = kDecNothing;
      return;
    }
  }
  if (!kRing && rf >= p.frames) {  // the reference lies past the caller's tensor
    *st = kDecMalformed;
    return;
  }
  if (last == kNull || rf == kNull) ref = 0;  // recv_inputs[NULL_FRAME] is the zeroed input
  // the frames this call may write: above `last` (protocol.rs:661-663), never below 0, and
  // below `frames` (linear) or the first R of them (ring: no slot twice)
  const int64_t wlo = last < 0 ? 0 : static_cast<int64_t>(last) + 1;
  const int64_t whi = kRing ? (start > wlo ? start : wlo) + rmask : static_cast<int64_t>(p.frames) - 1;
  int32_t newest = last;
  auto put = [&](int64_t f, uint32_t v) __attribute__((always_inline)) {
    if (f >= wlo && f <= whi) {
      const size_t slot = kRing ? (static_cast<uint32_t>(f) & rmask) : static_cast<size_t>(f);
      col[slot * plane] = static_cast<T>(v);
      newest = static_cast<int32_t>(f);
    }
  };
  uint32_t w0[8] = {head0.x, head0.y, head0.z, head0.w, head1.x, head1.y, head1.z, head1.w};
  // The two shapes a tick's packet almost always has (p2p.hpp wire_poll): one literal of every byte,
  // or one compressed run.  Both are valid by their header alone: one pass, no general parse.
  {
    const uint32_t h0 = w0[0] & 0xFFu;
    const bool lit = !(h0 & 0x81u) && static_cast<int32_t>(h0 >> 1) == n - 1 && n <= 32 && (n - 1) % IB == 0;
    const bool run = (h0 & 0x81u) == 1u && n == 1 && (h0 >> 2) % IB == 0;
    if (lit || run) {
      const int32_t nb = lit ? n - 1 : static_cast<int32_t>(h0 >> 2);
      const uint32_t fill = (h0 & 2u) ? 0xFFu : 0u;
      uint32_t win[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) win[i] = w0[i];
      window_shift(win);  // skip the header
      uint32_t acc = 0;
      for (int32_t k = 0; k < nb; ++k) {
        const uint32_t x = lit ? (win[0] & 0xFFu) : fill;
        if (lit) window_shift(win);
        const int i = k % IB;
        acc |= (((ref >> (8 * i)) ^ x) & 0xFFu) << (8 * i);
        if (i == IB - 1) {
          put(start + static_cast<int64_t>(k / IB), acc);
          acc = 0;
        }
      }
      p.upto[e] = newest;
      *st = newest == last ? kDecNothing : kDecOk;
      return;
    }
  }
  // The general packet: pass 0 validates without writing (a malformed packet leaves the tensor as
  // it was, protocol.rs:656), pass 1 writes.  Bytes past the 32 of the window are loaded one by one.
  for (int pass = 0; pass < 2; ++pass) {
    uint32_t win[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) win[i] = w0[i];
    int32_t pos = 0;
    uint32_t k = 0, acc = 0;  // k: bytes of the XOR stream so far (mod 2^32: pass 0 reads its remainder by IB)
    bool ok = true, past = false;
    auto next = [&]() __attribute__((always_inline)) -> uint32_t {
      const uint32_t b = pos < 32 ? (win[0] & 0xFFu) : pk[pos];
      window_shift(win);
      ++pos;
      return b;
    };
    auto emit = [&](uint32_t x) __attribute__((always_inline)) {
      const uint32_t i = k % IB;
      acc |= (((ref >> (8 * i)) ^ x) & 0xFFu) << (8 * i);
      if (i == IB - 1) {
        const int64_t f = start + static_cast<int64_t>(k / IB);
        put(f, acc);
        past = f >= whi;  // nothing after this frame is written: the rest of the packet is validated already
        acc = 0;
      }
      ++k;
    };
    while (pos < n && !past) {
      uint32_t hdr;
      if (!rb_wire::varint_get(pos, n, next, hdr)) {  // LEB128 (wire_varint.hpp)
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
          k += len;
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
        for (uint32_t i = 0; i < len && !past; ++i) {
          const uint32_t x = next();
          if (pass == 1) emit(x);
          else ++k;
        }
      }
    }
    if (pass == 0 && (!ok || k % IB != 0)) {  // compression.rs:47: whole inputs only
      *st = kDecMalformed;
      return;
    }
  }
  p.upto[e] = newest;
  *st = newest == last ? kDecNothing : kDecOk;
}

template <int IB, bool kRing>
__global__ void __launch_bounds__(256) decode_packets_all_kernel(const DecAllParams p) {
  const int s = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= p.S) return;
  decode_endpoint<IB, kRing>(p, static_cast<int>((p.handles >> (8 * blockIdx.y)) & 0xFFu), s);
}

struct EncAllParams {
  const uint8_t* inputs;  // [frames][P][S] Input values of IB bytes
  const int32_t* acked;   // [P][S]
  const int32_t* newest;  // [P][S]
  uint8_t* packets;       // [P][S] rows of packet_stride bytes
  int64_t packet_stride;
  int32_t* lengths;       // [P][S]
  int32_t* start_frames;  // [P][S]
  int32_t P, S, frames, first_frame;
  uint32_t handles;  // pack_handles
};

constexpr int32_t kEncNothing = 0, kEncTooLong = -1, kEncOverrun = -2;
constexpr int kEncAhead = 4;  // inputs loaded ahead of the scan

// UdpProtocol::send_pending_output for the endpoint of handle h, session s
template <int IB, bool kRing>
__device__ __forceinline__ void encode_endpoint(const EncAllParams& p, int h, int s) {
  using T = typename InputWord<IB>::type;
  const size_t e = static_cast<size_t>(h) * p.S + s;
  const uint32_t rmask = static_cast<uint32_t>(p.frames) - 1u;
  const T* const col = reinterpret_cast<const T*>(p.inputs) + e;
  const size_t plane = static_cast<size_t>(p.P) * p.S;
  const int32_t acked = p.acked[e], newest = p.newest[e];
  // pending_output starts after the last ack, or at the sender's first input before any ack
  // (protocol.rs:471-476)
  const int64_t start = acked == kNull ? p.first_frame : static_cast<int64_t>(acked) + 1;
  p.start_frames[e] = static_cast<int32_t>(start);
  if (newest < start || start < 0 || (!kRing && newest >= p.frames)) {
    p.lengths[e] = kEncNothing;
    return;
  }
  // from here 0 <= start <= newest, and acked is NULL_FRAME or start - 1 >= 0
  const uint32_t count = static_cast<uint32_t>(newest - start) + 1u;  // inputs to send
  if (kRing && count + (acked != kNull ? 1u : 0u) > rmask + 1u) {
    p.lengths[e] = kEncOverrun;  // the reference input's slot holds a newer frame by now
    return;
  }
  auto load = [&](uint32_t i) __attribute__((always_inline)) -> uint32_t {  // input i of the packet, i < count
    const int64_t f = start + i;
    const size_t slot = kRing ? (static_cast<uint32_t>(f) & rmask) : static_cast<size_t>(f);
    return col[slot * plane];
  };
  // one round trip: the reference and the first inputs (indices clamped to the packet's last)
  const size_t aslot = kRing ? (static_cast<uint32_t>(acked) & rmask) : static_cast<size_t>(acked < 0 ? 0 : acked);
  uint32_t ref = col[aslot * plane];
  uint32_t first[kEncAhead], pre[kEncAhead];
#pragma unroll
  for (int i = 0; i < kEncAhead; ++i) pre[i] = first[i] = load(static_cast<uint32_t>(i) < count ? i : count - 1);
  if (acked == kNull) ref = 0;
#pragma unroll
  for (int i = 0; i < kEncAhead; ++i) first[i] ^= ref;

  uint8_t* const out = p.packets + static_cast<int64_t>(e) * p.packet_stride;
  const int64_t cap = p.packet_stride;
  uint32_t win[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // the packet's first 32 bytes, shifted in from the top
  int32_t pos = 0;
  bool ok = true;
  auto put = [&](uint32_t b) __attribute__((always_inline)) {
    if (pos >= cap) {
      ok = false;
      return;
    }
    if (pos < 32) {
      window_shift(win);
      win[7] |= b << 24;
    } else {
      out[pos] = static_cast<uint8_t>(b);
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
  // byte a .. b - 1 of the XOR stream as one literal segment (read again: the first inputs from
  // registers, later ones from the cache the scan just filled)
  auto flush = [&](uint32_t a, uint32_t b) __attribute__((always_inline)) {
    if (b <= a) return;
    put_header((b - a) << 1);
    uint32_t at = ~0u, word = 0;
    for (uint32_t i = a; i < b && ok; ++i) {
      const uint32_t fi = i / IB;
      if (fi != at) {
        at = fi;
        word = fi == 0 ? first[0] : fi == 1 ? first[1] : fi == 2 ? first[2] : fi == 3 ? first[3] : (load(fi) ^ ref);
      }
      put((word >> (8 * (i % IB))) & 0xFFu);
    }
  };
  // One scan over the stream's bytes: a maximal run of >= kRunMin equal 0x00 / 0xFF bytes becomes a
  // compressed segment, everything between two of them one literal (the oracle's wire::rle_encode).
  const uint32_t total = count * IB;
  uint32_t lit = 0, run_at = 0, run_byte = 0x100u, word = 0;
  auto close_run = [&](uint32_t end) __attribute__((always_inline)) {
    if ((run_byte == 0u || run_byte == 0xFFu) && end - run_at >= static_cast<uint32_t>(kRunMin)) {
      flush(lit, run_at);
      put_header(((end - run_at) << 2) | (run_byte ? 2u : 0u) | 1u);
      lit = end;
    }
  };
  for (uint32_t k = 0; k < total && ok; ++k) {
    if (k % IB == 0) {  // the next input, and a load kEncAhead inputs ahead of it
      const uint32_t fi = k / IB;
      word = pre[0] ^ ref;
#pragma unroll
      for (int i = 0; i < kEncAhead - 1; ++i) pre[i] = pre[i + 1];
      pre[kEncAhead - 1] = load(fi + kEncAhead < count ? fi + kEncAhead : count - 1);
    }
    const uint32_t b = (word >> (8 * (k % IB))) & 0xFFu;
    if (b != run_byte) {
      close_run(k);
      run_at = k;
      run_byte = b;
    }
  }
  if (ok) close_run(total);
  if (ok) flush(lit, total);
  if (!ok) {
    p.lengths[e] = kEncTooLong;  // the packet does not fit packet_stride
    return;
  }
  // bring byte 0 down to the window's first byte: (32 - pos) bytes to drop, pos >= 1
  if (pos < 32) {
    const uint32_t m = 32u - static_cast<uint32_t>(pos);
    if (m & 16u) {
#pragma unroll
      for (int i = 0; i < 4; ++i) win[i] = win[i + 4], win[i + 4] = 0;
    }
    if (m & 8u) {
#pragma unroll
      for (int i = 0; i < 8; ++i) win[i] = i + 2 < 8 ? win[i + 2] : 0u;
    }
    if (m & 4u) {
#pragma unroll
      for (int i = 0; i < 8; ++i) win[i] = i + 1 < 8 ? win[i + 1] : 0u;
    }
    const uint32_t r = m & 3u;
#pragma unroll
    for (int i = 0; i < 7; ++i) win[i] = __builtin_amdgcn_alignbyte(win[i + 1], win[i], r);
    win[7] >>= 8 * r;
  }
  reinterpret_cast<uint4*>(out)[0] = make_uint4(win[0], win[1], win[2], win[3]);
  if (pos > 16) reinterpret_cast<uint4*>(out)[1] = make_uint4(win[4], win[5], win[6], win[7]);
  p.lengths[e] = pos;
}

template <int IB, bool kRing>
__global__ void __launch_bounds__(256) encode_packets_all_kernel(const EncAllParams p) {
  const int s = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= p.S) return;
  encode_endpoint<IB, kRing>(p, static_cast<int>((p.handles >> (8 * blockIdx.y)) & 0xFFu), s);
}

bool all_args_ok(uint32_t handle_mask, int32_t num_players, int32_t num_sessions, int32_t input_bytes,
                 const void* packets, int64_t packet_stride, int32_t frames, int32_t ring_frames) {
  if (num_players <= 0 || num_players > 4 || num_sessions <= 0) return false;
  if (handle_mask == 0 || (handle_mask >> num_players) != 0) return false;
  if (input_bytes != 1 && input_bytes != 2 && input_bytes != 4) return false;
  if (packet_stride < 32 || packet_stride % 16 != 0 || reinterpret_cast<uintptr_t>(packets) % 16 != 0) return false;
  if (frames <= 0) return false;
  if (ring_frames != 0 && (ring_frames < 128 || (ring_frames & (ring_frames - 1)) != 0 || frames != ring_frames))
    return false;
  return true;
}

// one instantiation per input size and layout: the slot arithmetic and the store width are the kernel's
#define RB_LAUNCH_BY_SHAPE(kernel, input_bytes, ring, grid, stream, params)                                  \
  do {                                                                                                     \
    if (ring) {                                                                                            \
      if ((input_bytes) == 1) hipLaunchKernelGGL((kernel<1, true>), grid, dim3(256), 0, stream, params);   \
      else if ((input_bytes) == 2) hipLaunchKernelGGL((kernel<2, true>), grid, dim3(256), 0, stream, params); \
      else hipLaunchKernelGGL((kernel<4, true>), grid, dim3(256), 0, stream, params);                      \
    } else {                                                                                               \
      if ((input_bytes) == 1) hipLaunchKernelGGL((kernel<1, false>), grid, dim3(256), 0, stream, params);  \
      else if ((input_bytes) == 2) hipLaunchKernelGGL((kernel<2, false>), grid, dim3(256), 0, stream, params); \
      else hipLaunchKernelGGL((kernel<4, false>), grid, dim3(256), 0, stream, params);                     \
    }                                                                                                      \
  } while (0)

}  // namespace

extern "C" {

rb_status rb_decode_input_packets(int32_t device, void* stream, int32_t handle, int32_t num_players,
                                  int32_t num_sessions, int32_t input_bytes, int32_t max_prediction,
                                  const uint8_t* packets, int64_t packet_stride, const int32_t* lengths,
                                  const int32_t* start_frames, void* remote_inputs, int32_t remote_frames,
                                  int32_t* remote_upto, int32_t* status) {
  if (handle < 0 || handle >= num_players || num_players > 4 || num_sessions <= 0 ||
      (input_bytes != 1 && input_bytes != 2 && input_bytes != 4) || max_prediction <= 0)
    return RB_INVALID_REQUEST;
  if (hipSetDevice(device) != hipSuccess) return RB_DEVICE_ERROR;
  DecParams p{packets, packet_stride, lengths, start_frames, static_cast<uint8_t*>(remote_inputs), remote_upto,
              status, handle, num_players, num_sessions, input_bytes, remote_frames, max_prediction};
  hipLaunchKernelGGL(decode_packets_kernel, dim3((num_sessions + 255) / 256), dim3(256), 0,
                     static_cast<hipStream_t>(stream), p);
  return hipGetLastError() == hipSuccess ? RB_OK : RB_DEVICE_ERROR;
}

rb_status rb_encode_input_packets(int32_t device, void* stream, int32_t handle, int32_t num_players,
                                  int32_t num_sessions, int32_t input_bytes, const void* inputs, int32_t frames,
                                  int32_t first_frame, const int32_t* acked, const int32_t* newest, uint8_t* packets,
                                  int64_t packet_stride, int32_t* lengths, int32_t* start_frames) {
  if (handle < 0 || handle >= num_players || num_players > 4 || num_sessions <= 0 ||
      (input_bytes != 1 && input_bytes != 2 && input_bytes != 4) || packet_stride <= 0)
    return RB_INVALID_REQUEST;
  if (hipSetDevice(device) != hipSuccess) return RB_DEVICE_ERROR;
  EncParams p{static_cast<const uint8_t*>(inputs), frames, acked, newest, packets, packet_stride, lengths,
              start_frames, handle, num_players, num_sessions, input_bytes, first_frame};
  hipLaunchKernelGGL(encode_packets_kernel, dim3((num_sessions + 255) / 256), dim3(256), 0,
                     static_cast<hipStream_t>(stream), p);
  return hipGetLastError() == hipSuccess ? RB_OK : RB_DEVICE_ERROR;
}

rb_status rb_decode_input_packets_all(int32_t device, void* stream, uint32_t handle_mask, int32_t num_players,
                                      int32_t num_sessions, int32_t input_bytes, int32_t max_prediction,
                                      const uint8_t* packets, int64_t packet_stride, const int32_t* lengths,
                                      const int32_t* start_frames, void* inputs, int32_t frames, int32_t ring_frames,
                                      int32_t* upto, int32_t* status) {
  if (!all_args_ok(handle_mask, num_players, num_sessions, input_bytes, packets, packet_stride, frames, ring_frames) ||
      max_prediction <= 0)
    return RB_INVALID_REQUEST;
  // a packet's reference input may be 2*max_prediction frames old and must still be in the ring
  if (ring_frames != 0 && 2 * static_cast<int64_t>(max_prediction) >= ring_frames) return RB_INVALID_REQUEST;
  if (hipSetDevice(device) != hipSuccess) return RB_DEVICE_ERROR;
  int count = 0;
  const uint32_t handles = pack_handles(handle_mask, count);
  DecAllParams p{packets, packet_stride, lengths, start_frames, static_cast<uint8_t*>(inputs), upto, status,
                 num_players, num_sessions, frames, max_prediction, handles};
  const dim3 grid((num_sessions + 255) / 256, count);
  RB_LAUNCH_BY_SHAPE(decode_packets_all_kernel, input_bytes, ring_frames != 0, grid, static_cast<hipStream_t>(stream), p);
  return hipGetLastError() == hipSuccess ? RB_OK : RB_DEVICE_ERROR;
}

rb_status rb_encode_input_packets_all(int32_t device, void* stream, uint32_t handle_mask, int32_t num_players,
                                      int32_t num_sessions, int32_t input_bytes, const void* inputs, int32_t frames,
                                      int32_t ring_frames, int32_t first_frame, const int32_t* acked,
                                      const int32_t* newest, uint8_t* packets, int64_t packet_stride, int32_t* lengths,
                                      int32_t* start_frames) {
  if (!all_args_ok(handle_mask, num_players, num_sessions, input_bytes, packets, packet_stride, frames, ring_frames))
    return RB_INVALID_REQUEST;
  if (hipSetDevice(device) != hipSuccess) return RB_DEVICE_ERROR;
  int count = 0;
  const uint32_t handles = pack_handles(handle_mask, count);
  EncAllParams p{static_cast<const uint8_t*>(inputs), acked, newest, packets, packet_stride, lengths, start_frames,
                 num_players, num_sessions, frames, first_frame, handles};
  const dim3 grid((num_sessions + 255) / 256, count);
  RB_LAUNCH_BY_SHAPE(encode_packets_all_kernel, input_bytes, ring_frames != 0, grid, static_cast<hipStream_t>(stream), p);
  return hipGetLastError() == hipSuccess ? RB_OK : RB_DEVICE_ERROR;
}

}  // extern "C"
