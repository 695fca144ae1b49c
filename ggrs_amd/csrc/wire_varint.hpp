// ggrs_amd/csrc/wire_varint.hpp — the one LEB128 header parser of the packet format
// (network/compression.rs over bitfield-rle), shared by the stand-alone decoder
// (wire.hip) and the decoder inside the P2P tick (p2p.hpp wire_poll).
//
// It accepts exactly what the oracle's 64-bit accumulator (oracle/ggrs_oracle.hpp
// wire::varint_get followed by rle_decode's length checks) accepts:
//   * up to ten bytes; a header still continued after the tenth, or cut off by the end of
//     the packet, is malformed;
//   * a value that reaches 2^32 is malformed: it is neither a run of at most 65,536 bytes
//     nor a literal that fits a packet.  So bits 32-34 of the fifth byte, any payload bit
//     of bytes six to nine and bit 0 of the tenth (bit 63) make the header malformed;
//   * continuation groups past the fifth byte whose payload bits are zero (a padded,
//     non-canonical header) change nothing and are accepted; bits 1-6 of the tenth byte
//     lie past bit 63 and are dropped, as the 64-bit shift drops them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rb_wire {

// `pos` is the caller's read position and `n` the packet's length; next() returns the byte
// at `pos` and advances it.  False: malformed (truncated, over-long, or a value >= 2^32).
template <class Next>
__device__ __forceinline__ bool varint_get(const int32_t& pos, int32_t n, Next&& next, uint32_t& hdr) {
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

}  // namespace rb_wire
