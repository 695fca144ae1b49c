// ggrs_amd/csrc/time_sync.hpp — the batched time sync of P2P batches
// (include/ggrs_amd.h rb_p2p_time_sync_enable): TimeSync (time_sync.rs),
// UdpProtocol::update_local_frame_advantage (protocol.rs:268-277), the window
// write of send_input (protocol.rs:439-455) and the session's
// max_frame_advantage / check_wait_recommendation (p2p_session.rs:745-776).
//
// Time sync never feeds back into a session inside a launch: it produces
// frames_ahead, WaitRecommendation events and the per-endpoint advantages, and
// a caller can act on them only between launches.  So it is a function of what
// each tick already knows, and runs as a kernel of its own after the P2P
// launch, on the tick log that launch wrote (p2p.hpp kTl*, p2p_kernel kLog).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "p2p.hpp"

namespace rb {

constexpr int kTsWindow = 30;            // time_sync.rs:3 FRAME_WINDOW_SIZE
constexpr int32_t kTsMinRecommend = 3;   // p2p_session.rs:24 MIN_RECOMMENDATION
constexpr int32_t kTsInterval = 60;      // p2p_session.rs:23 RECOMMENDATION_INTERVAL
constexpr int kTsEvents = 8;             // = RB_P2P_WAIT_EVENTS_KEPT

// TimeSync::average_frame_advantage (time_sync.rs:30-39) from the two windows' sums: the averages
// in f32, IEEE divisions, the cast truncating towards zero (Rust's `as i32`; the quotient of two
// i32 sums is far inside i32, so the saturating cases of `as` cannot occur).
__host__ __device__ inline int32_t time_sync_average(int32_t local_sum, int32_t remote_sum) {
  const float local_avg = static_cast<float>(local_sum) / static_cast<float>(kTsWindow);
  const float remote_avg = static_cast<float>(remote_sum) / static_cast<float>(kTsWindow);
  return static_cast<int32_t>((remote_avg - local_avg) / 2.0f);
}

// The per-session rows [TS_ROWS][Spad] (one word per session each; handle h of a 4-wide group at +h)
enum TsRow : int {
  TS_LOCAL_ADV = 0,     // UdpProtocol::local_frame_advantage
  TS_REMOTE_ADV = 4,    // UdpProtocol::remote_frame_advantage (the peer's QualityReport)
  TS_RTT = 8,           // UdpProtocol::round_trip_time, milliseconds (the QualityReply)
  TS_LOCAL_SUM = 12,    // sum of the local window (kept running: sum += new - old)
  TS_REMOTE_SUM = 16,
  TS_NEXT_SLEEP = 20,   // P2PSession::next_recommended_sleep
  TS_FRAMES_AHEAD = 21, // P2PSession::frames_ahead
  TS_EV_N = 22,         // WaitRecommendation events since enable
  TS_EV_FRAME = 24,     // [kTsEvents] ring, slot = event index % kTsEvents: current_frame of the event
  TS_EV_SKIP = 32,      // [kTsEvents] its skip_frames
  TS_ROWS = 40
};

struct TimeSyncParams {
  int32_t* state;  // [TS_ROWS][Spad]
  int32_t* win;    // [2 local, remote][kTsWindow][4 handles][Spad]
  int32_t fps;
};

__host__ __device__ inline size_t ts_win_index(int which, int slot, int h, size_t Spad, size_t s) {
  return ((static_cast<size_t>(which) * kTsWindow + static_cast<size_t>(slot)) * 4 + static_cast<size_t>(h)) * Spad + s;
}

// One thread per session: the launch's ticks in order, the session's time-sync state in registers
// from entry to exit, the windows in HBM (one read and one write per window, handle and tick that
// reaches send_input).  Each consumed log row is marked unwritten again, so a row the next P2P
// launch does not write (a session stopped on a panic) ends the walk.
//
// A batch of 65,536 sessions is one wave per SIMD here, and a tick's steps depend on each other
// through memory (the log row, then the window slot it names), so the walk is latency bound.  The
// ticks go in chunks of kTsChunk: the chunk's log rows and delivery watermarks are loaded together
// (addresses known up front), then the old values of the window slots its ticks may write.  Those
// slots are distinct inside a chunk: only a tick that reaches send_input writes, each such tick
// moves current_frame on by one, and a chunk is shorter than the window.
constexpr int kTsChunk = 10;
static_assert(kTsChunk < kTsWindow, "a chunk's window slots must be distinct");

template <int P>
__global__ void __launch_bounds__(256)
p2p_time_sync_kernel(const TimeSyncParams ts, int32_t* __restrict__ log, int64_t log_stride,
                     const int32_t* __restrict__ upto, int64_t upto_stride, const int32_t* __restrict__ status, int T,
                     int S, int Spad, int32_t remote_frames, uint32_t local_mask, int32_t delay, int peer_on) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const size_t sp = static_cast<size_t>(Spad);
  auto row = [&](int r) -> int32_t& { return ts.state[static_cast<size_t>(r) * sp + s]; };
  int32_t ladv[P], radv[P], rtt[P], lsum[P], rsum[P];
#pragma unroll
  for (int h = 0; h < P; ++h) {
    ladv[h] = row(TS_LOCAL_ADV + h);
    radv[h] = row(TS_REMOTE_ADV + h);
    rtt[h] = row(TS_RTT + h);
    lsum[h] = row(TS_LOCAL_SUM + h);
    rsum[h] = row(TS_REMOTE_SUM + h);
  }
  int32_t next_sleep = row(TS_NEXT_SLEEP), frames_ahead = row(TS_FRAMES_AHEAD);
  uint32_t ev_n = static_cast<uint32_t>(row(TS_EV_N));
  // a session whose last advance_frame panicked: its last written row is the tick that panicked
  // (a panic after the threshold decision leaves that row's own mark at Ok)
  const bool panicked = status[s] == kP2PStatusPanic;
  // the window slot of the input a tick at frame `cur` sends (cur >= 0; the unsigned form keeps the
  // slot of an unwritten row's stale word in range)
  auto slot_of = [&](int32_t cur) { return static_cast<int>(static_cast<uint32_t>(cur + delay) % static_cast<uint32_t>(kTsWindow)); };
  bool stop = false;
  for (int t0 = 0; t0 < T && !stop; t0 += kTsChunk) {
    int32_t endv[kTsChunk], curv[kTsChunk], upv[kTsChunk][P], wl[kTsChunk][P], wr[kTsChunk][P];
    uint32_t entv[kTsChunk];
#pragma unroll
    for (int k = 0; k < kTsChunk; ++k) {  // (rows past the launch's last: that row again, never used)
      const int64_t tt = min(t0 + k, T - 1);
      const int32_t* const lr = log + tt * log_stride;
      endv[k] = lr[kTlEnd * sp + s];
      curv[k] = lr[kTlCur * sp + s];
      entv[k] = peer_on ? static_cast<uint32_t>(lr[kTlEntry * sp + s]) : 0u;
#pragma unroll
      for (int h = 0; h < P; ++h)
        upv[k][h] = ((local_mask >> h) & 1u) ? kNullFrame : upto[tt * upto_stride + static_cast<int64_t>(h) * S + s];
    }
    const int32_t end_after = t0 + kTsChunk < T ? log[static_cast<int64_t>(t0 + kTsChunk) * log_stride + kTlEnd * sp + s] : kTlUnwritten;
#pragma unroll
    for (int k = 0; k < kTsChunk; ++k) {
      const int slot = slot_of(curv[k]);
#pragma unroll
      for (int h = 0; h < P; ++h) {
        wl[k][h] = ((local_mask >> h) & 1u) ? 0 : ts.win[ts_win_index(0, slot, h, sp, s)];
        wr[k][h] = ((local_mask >> h) & 1u) ? 0 : ts.win[ts_win_index(1, slot, h, sp, s)];
      }
    }
    // tick t0 + k of the chunk (a lambda per tick, so that the loop over k unrolls and the chunk's
    // values stay in registers)
    auto tick = [&](int k) __attribute__((always_inline)) {
      const int t = t0 + k;
      if (t >= T || stop) return;
      const int32_t end = endv[k];
      if (end == kTlUnwritten) {
        stop = true;
        return;
      }
      const int32_t end_n = t + 1 >= T ? kTlUnwritten : k + 1 < kTsChunk ? endv[min(k + 1, kTsChunk - 1)] : end_after;
      const int32_t cur = curv[k];
      const uint32_t after = (static_cast<uint32_t>(end) >> 4) & 0xFu;
      const uint32_t entry = peer_on ? entv[k] : after;
      log[static_cast<int64_t>(t) * log_stride + kTlEnd * sp + s] = kTlUnwritten;
      // poll_remote_clients (p2p_session.rs:387-392): update_local_frame_advantage of every running endpoint
#pragma unroll
      for (int h = 0; h < P; ++h) {
        if (((local_mask | entry) >> h) & 1u) continue;
        const int32_t last_recv = min(upv[k][h], remote_frames - 1);
        if (last_recv == kNullFrame) continue;
        const int32_t ping = rtt[h] / 2;
        ladv[h] = last_recv + (ping * ts.fps) / 1000 - cur;
      }
      if ((static_cast<uint32_t>(end) & 3u) == kTlPanic || (panicked && end_n == kTlUnwritten)) {
        stop = true;
        return;
      }
      // check_wait_recommendation (p2p_session.rs:763-776) over max_frame_advantage (:745-761)
      int32_t fa = INT32_MIN;
#pragma unroll
      for (int h = 0; h < P; ++h)
        if (!(((local_mask | after) >> h) & 1u)) fa = max(fa, time_sync_average(lsum[h], rsum[h]));
      frames_ahead = fa == INT32_MIN ? 0 : fa;
      if (cur > next_sleep && frames_ahead >= kTsMinRecommend) {
        next_sleep = cur + kTsInterval;
        const uint32_t slot = ev_n % kTsEvents;
        row(TS_EV_FRAME + static_cast<int>(slot)) = cur;
        row(TS_EV_SKIP + static_cast<int>(slot)) = frames_ahead;
        ++ev_n;
      }
      // send_input (protocol.rs:439-455), reached only past add_local_input: TimeSync::advance_frame
      // at the local input's frame
      if ((static_cast<uint32_t>(end) & 3u) == kTlOk) {
        const int slot = slot_of(cur);
#pragma unroll
        for (int h = 0; h < P; ++h) {
          if (((local_mask | after) >> h) & 1u) continue;
          lsum[h] += ladv[h] - wl[k][h];
          rsum[h] += radv[h] - wr[k][h];
          ts.win[ts_win_index(0, slot, h, sp, s)] = ladv[h];
          ts.win[ts_win_index(1, slot, h, sp, s)] = radv[h];
        }
      }
    };
#pragma unroll
    for (int k = 0; k < kTsChunk; ++k) tick(k);
  }
#pragma unroll
  for (int h = 0; h < P; ++h) {
    row(TS_LOCAL_ADV + h) = ladv[h];
    row(TS_LOCAL_SUM + h) = lsum[h];
    row(TS_REMOTE_SUM + h) = rsum[h];
  }
  row(TS_NEXT_SLEEP) = next_sleep;
  row(TS_FRAMES_AHEAD) = frames_ahead;
  row(TS_EV_N) = static_cast<int32_t>(ev_n);
}

// on_quality_reply / on_quality_report (protocol.rs:697-708) for the endpoint of remote handle h
__global__ void p2p_receive_quality_kernel(const TimeSyncParams ts, const int32_t* __restrict__ rtt_ms,
                                           const int32_t* __restrict__ frame_advantage, int S, int Spad, int h) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const size_t sp = static_cast<size_t>(Spad);
  if (rtt_ms) ts.state[static_cast<size_t>(TS_RTT + h) * sp + s] = rtt_ms[s];
  if (frame_advantage) ts.state[static_cast<size_t>(TS_REMOTE_ADV + h) * sp + s] = frame_advantage[s];
}

// frames_ahead [S] and local_frame_advantage [P][S] (the QualityReport payload) to the caller's device memory
__global__ void p2p_export_time_sync_kernel(const TimeSyncParams ts, int32_t* __restrict__ frames_ahead,
                                            int32_t* __restrict__ local_adv, int S, int Spad, int P) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const size_t sp = static_cast<size_t>(Spad);
  if (frames_ahead) frames_ahead[s] = ts.state[static_cast<size_t>(TS_FRAMES_AHEAD) * sp + s];
  if (local_adv)
    for (int h = 0; h < P; ++h) local_adv[static_cast<size_t>(h) * S + s] = ts.state[static_cast<size_t>(TS_LOCAL_ADV + h) * sp + s];
}

__global__ void time_sync_average_kernel(const int32_t* __restrict__ local_sums, const int32_t* __restrict__ remote_sums,
                                         int32_t* __restrict__ out, int64_t n) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) out[i] = time_sync_average(local_sums[i], remote_sums[i]);
}

}  // namespace rb
