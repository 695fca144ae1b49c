// ggrs_amd/csrc/wire_group.hip — the packet codec for endpoints that carry several handles in one
// stream (rb_decode_input_packets_grouped / rb_encode_input_packets_grouped):
// a remote peer with more than one local player, and every spectator endpoint.
//
// One lane per endpoint, group-major: blockIdx.y walks the groups of one size, so a wave holds 64
// consecutive sessions of one group and each member's loads and stores of one frame are one row of
// the tensor.  One instantiation per input size, group size and layout: the frame's width and the
// members' places in it are constants (wire_group_step.hpp), nothing is indexed by a register.
// A call with groups of two sizes is two launches.
//
// As in wire.hip, frame arithmetic is 64-bit and every tensor index is either masked (ring) or
// range-checked (linear) right where it is formed: addresses stay inside the tensors whatever the
// lengths, start frames, watermarks and packet bytes hold.
#include <hip/hip_runtime.h>

#include "../../include/ggrs_amd.h"
#include "wire_group_step.hpp"

namespace {

template <int IB> struct InputWord;
template <> struct InputWord<1> { using type = uint8_t; };
template <> struct InputWord<2> { using type = uint16_t; };
template <> struct InputWord<4> { using type = uint32_t; };

struct GroupList {
  uint32_t members[4];  // per group of this launch: its handles, one per byte, lowest (the lead) first
};

struct DecGroupParams {
  const uint8_t* packets;  // [P][S] rows of packet_stride bytes
  int64_t packet_stride;
  const int32_t* lengths;       // [P][S]
  const int32_t* start_frames;  // [P][S]
  uint8_t* inputs;              // [frames][P][S] Input values of IB bytes
  int32_t* upto;                // [P][S]
  int32_t* status;              // [P][S]
  int32_t P, S, frames, max_prediction;
  GroupList groups;
};

template <int IB, int K>
struct DecIo {
  using T = typename InputWord<IB>::type;
  T* base;  // frame / slot 0, handle 0 of this session
  size_t plane, member[K];
  const uint8_t* pk;
  __device__ __forceinline__ uint32_t load(int m, size_t slot) const { return base[slot * plane + member[m]]; }
  __device__ __forceinline__ void store(int m, size_t slot, uint32_t v) const { base[slot * plane + member[m]] = static_cast<T>(v); }
  __device__ __forceinline__ void chunk(int32_t off, uint32_t (&w)[4]) const {
    const uint4 c = *reinterpret_cast<const uint4*>(pk + off);
    w[0] = c.x, w[1] = c.y, w[2] = c.z, w[3] = c.w;
  }
};

template <int IB, int K, bool kRing>
__global__ void __launch_bounds__(256) decode_packets_grouped_kernel(const DecGroupParams p) {
  const int s = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= p.S) return;
  const uint32_t mem = p.groups.members[blockIdx.y];
  const size_t e = static_cast<size_t>(mem & 0xFFu) * p.S + s;  // the lead's row
  // every load whose address the lane knows: lengths, start frame, watermark, the packet's head
  int32_t n = p.lengths[e], start = p.start_frames[e], last = p.upto[e];
  const uint8_t* pk = p.packets + static_cast<int64_t>(e) * p.packet_stride;
  uint4 head0 = reinterpret_cast<const uint4*>(pk)[0], head1 = reinterpret_cast<const uint4*>(pk)[1];
  // all five loads are in flight before the first is waited for (wire.hip decode_endpoint)
  asm volatile("" : "+v"(n), "+v"(start), "+v"(last), "+v"(head0.x), "+v"(head0.y), "+v"(head0.z), "+v"(head0.w),
               "+v"(head1.x), "+v"(head1.y), "+v"(head1.z), "+v"(head1.w));
  DecIo<IB, K> io;
  io.base = reinterpret_cast<typename InputWord<IB>::type*>(p.inputs) + s;
  io.plane = static_cast<size_t>(p.P) * p.S;
  io.pk = pk;
#pragma unroll
  for (int m = 0; m < K; ++m) io.member[m] = static_cast<size_t>((mem >> (8 * m)) & 0xFFu) * p.S;
  const uint32_t head[8] = {head0.x, head0.y, head0.z, head0.w, head1.x, head1.y, head1.z, head1.w};
  int32_t newest;
  bool decoded;
  const int32_t code = rb::wg_decode<IB, K, kRing>(io, n, start, last, head, p.packet_stride, p.frames, p.max_prediction,
                                                   newest, decoded);
  if (decoded) {  // every member's row: rb_p2p_run_ticks and rb_spectator_run_ticks read them as before
#pragma unroll
    for (int m = 0; m < K; ++m) p.upto[io.member[m] + s] = newest;
  }
  p.status[e] = code;
}

struct EncGroupParams {
  const uint8_t* inputs;  // [frames][P][S] Input values of IB bytes
  const int32_t* acked;   // [P][S]
  const int32_t* newest;  // [P][S]
  uint8_t* packets;       // [P][S] rows of packet_stride bytes
  int64_t packet_stride;
  int32_t* lengths;       // [P][S]
  int32_t* start_frames;  // [P][S]
  int32_t P, S, frames, first_frame;
  GroupList groups;
};

template <int IB, int K>
struct EncIo {
  using T = typename InputWord<IB>::type;
  const T* base;
  size_t plane, member[K];
  uint8_t* out;
  __device__ __forceinline__ uint32_t load(int m, size_t slot) const { return base[slot * plane + member[m]]; }
  __device__ __forceinline__ void store_byte(int32_t pos, uint32_t b) const { out[pos] = static_cast<uint8_t>(b); }
  __device__ __forceinline__ void store16(int i, const uint32_t (&w)[4]) const {
    reinterpret_cast<uint4*>(out)[i] = make_uint4(w[0], w[1], w[2], w[3]);
  }
};

template <int IB, int K, bool kRing>
__global__ void __launch_bounds__(256) encode_packets_grouped_kernel(const EncGroupParams p) {
  const int s = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= p.S) return;
  const uint32_t mem = p.groups.members[blockIdx.y];
  const size_t e = static_cast<size_t>(mem & 0xFFu) * p.S + s;
  const int32_t acked = p.acked[e], newest = p.newest[e];
  EncIo<IB, K> io;
  io.base = reinterpret_cast<const typename InputWord<IB>::type*>(p.inputs) + s;
  io.plane = static_cast<size_t>(p.P) * p.S;
  io.out = p.packets + static_cast<int64_t>(e) * p.packet_stride;
#pragma unroll
  for (int m = 0; m < K; ++m) io.member[m] = static_cast<size_t>((mem >> (8 * m)) & 0xFFu) * p.S;
  int32_t start;
  const int32_t length = rb::wg_encode<IB, K, kRing>(io, acked, newest, p.first_frame, p.frames, p.packet_stride, start);
  p.start_frames[e] = start;
  p.lengths[e] = length;
}

// the `_all` pair's rules (wire.hip all_args_ok) with groups in the mask's place
bool grouped_args_ok(uint32_t group_masks, int32_t num_players, int32_t num_sessions, int32_t input_bytes,
                     const void* packets, int64_t packet_stride, int32_t frames, int32_t ring_frames) {
  if (num_players <= 0 || num_players > 4 || num_sessions <= 0) return false;
  if (!rb::wg_groups_ok(group_masks, num_players)) return false;
  if (input_bytes != 1 && input_bytes != 2 && input_bytes != 4) return false;
  if (packet_stride < 32 || packet_stride % 16 != 0 || reinterpret_cast<uintptr_t>(packets) % 16 != 0) return false;
  if (frames <= 0) return false;
  if (ring_frames != 0 && (ring_frames < 128 || (ring_frames & (ring_frames - 1)) != 0 || frames != ring_frames))
    return false;
  return true;
}

// the groups of `size` handles, in the order the caller gave them
int groups_of_size(uint32_t group_masks, int size, GroupList& out) {
  int count = 0;
  for (int g = 0; g < 4; ++g) {
    const uint32_t mask = (group_masks >> (8 * g)) & 0xFFu;
    uint32_t packed = 0;
    int k = 0;
    for (uint32_t h = 0; h < 4; ++h)
      if ((mask >> h) & 1u) packed |= h << (8 * k++);
    if (k == size) out.members[count++] = packed;
  }
  for (int g = count; g < 4; ++g) out.members[g] = 0;
  return count;
}

#define RB_GROUP_LAUNCH_K(kernel, IB, K, ring, grid, stream, params)                                  \
  do {                                                                                              \
    if (ring) hipLaunchKernelGGL((kernel<IB, K, true>), grid, dim3(256), 0, stream, params);        \
    else hipLaunchKernelGGL((kernel<IB, K, false>), grid, dim3(256), 0, stream, params);            \
  } while (0)
#define RB_GROUP_LAUNCH_IB(kernel, input_bytes, K, ring, grid, stream, params)                       \
  do {                                                                                              \
    if ((input_bytes) == 1) RB_GROUP_LAUNCH_K(kernel, 1, K, ring, grid, stream, params);            \
    else if ((input_bytes) == 2) RB_GROUP_LAUNCH_K(kernel, 2, K, ring, grid, stream, params);       \
    else RB_GROUP_LAUNCH_K(kernel, 4, K, ring, grid, stream, params);                               \
  } while (0)
// one launch per group size present in the call
#define RB_GROUP_LAUNCH(kernel, group_masks, input_bytes, ring, num_sessions, stream, params)        \
  do {                                                                                              \
    for (int size = 1; size <= 4; ++size) {                                                         \
      const int count = groups_of_size(group_masks, size, (params).groups);                         \
      if (count == 0) continue;                                                                     \
      const dim3 grid(((num_sessions) + 255) / 256, count);                                         \
      if (size == 1) RB_GROUP_LAUNCH_IB(kernel, input_bytes, 1, ring, grid, stream, params);        \
      else if (size == 2) RB_GROUP_LAUNCH_IB(kernel, input_bytes, 2, ring, grid, stream, params);   \
      else if (size == 3) RB_GROUP_LAUNCH_IB(kernel, input_bytes, 3, ring, grid, stream, params);   \
      else RB_GROUP_LAUNCH_IB(kernel, input_bytes, 4, ring, grid, stream, params);                  \
    }                                                                                               \
  } while (0)

}  // namespace

extern "C" {

rb_status rb_decode_input_packets_grouped(int32_t device, void* stream, uint32_t group_masks, int32_t num_players,
                                          int32_t num_sessions, int32_t input_bytes, int32_t max_prediction,
                                          const uint8_t* packets, int64_t packet_stride, const int32_t* lengths,
                                          const int32_t* start_frames, void* inputs, int32_t frames, int32_t ring_frames,
                                          int32_t* upto, int32_t* status) {
  if (!grouped_args_ok(group_masks, num_players, num_sessions, input_bytes, packets, packet_stride, frames, ring_frames) ||
      max_prediction <= 0)
    return RB_INVALID_REQUEST;
  // a packet's reference input may be 2*max_prediction frames old and must still be in the ring
  if (ring_frames != 0 && 2 * static_cast<int64_t>(max_prediction) >= ring_frames) return RB_INVALID_REQUEST;
  if (hipSetDevice(device) != hipSuccess) return RB_DEVICE_ERROR;
  DecGroupParams p{packets, packet_stride, lengths, start_frames, static_cast<uint8_t*>(inputs), upto, status,
                   num_players, num_sessions, frames, max_prediction, {}};
  RB_GROUP_LAUNCH(decode_packets_grouped_kernel, group_masks, input_bytes, ring_frames != 0, num_sessions,
                  static_cast<hipStream_t>(stream), p);
  return hipGetLastError() == hipSuccess ? RB_OK : RB_DEVICE_ERROR;
}

rb_status rb_encode_input_packets_grouped(int32_t device, void* stream, uint32_t group_masks, int32_t num_players,
                                          int32_t num_sessions, int32_t input_bytes, const void* inputs, int32_t frames,
                                          int32_t ring_frames, int32_t first_frame, const int32_t* acked,
                                          const int32_t* newest, uint8_t* packets, int64_t packet_stride,
                                          int32_t* lengths, int32_t* start_frames) {
  if (!grouped_args_ok(group_masks, num_players, num_sessions, input_bytes, packets, packet_stride, frames, ring_frames))
    return RB_INVALID_REQUEST;
  if (hipSetDevice(device) != hipSuccess) return RB_DEVICE_ERROR;
  EncGroupParams p{static_cast<const uint8_t*>(inputs), acked, newest, packets, packet_stride, lengths, start_frames,
                   num_players, num_sessions, frames, first_frame, {}};
  RB_GROUP_LAUNCH(encode_packets_grouped_kernel, group_masks, input_bytes, ring_frames != 0, num_sessions,
                  static_cast<hipStream_t>(stream), p);
  return hipGetLastError() == hipSuccess ? RB_OK : RB_DEVICE_ERROR;
}

}  // extern "C"
