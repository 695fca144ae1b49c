// ggrs_amd/csrc/liveness.hpp — endpoint liveness of P2P batches
// (include/ggrs_amd.h rb_p2p_liveness_enable, rb_p2p_poll_liveness):
// UdpProtocol's two receive timers (network/protocol.rs:377-394), the stamp and NetworkResumed of
// handle_message (:555-562), on_input's disconnect_requested (:621-626) and the session's reaction
// (sessions/p2p_session.rs:818-847) for every remote endpoint of every session in one launch.
//
// No tick kernel reads these planes, and p2p.hpp is not touched: the kernel meets the ticks only
// in the write rb_p2p_disconnect_player already makes between them (p2p_disconnect_write, the one
// expression of it).  Game independent.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "liveness_step.hpp"
#include "p2p.hpp"

namespace rb {

constexpr int kLvEvents = 16;  // RB_P2P_NET_EVENTS_KEPT
enum { LV_EV_KIND = 0, LV_EV_HANDLE = 1, LV_EV_VALUE = 2, LV_EV_ROWS = 3 };

struct LivenessParams {
  int64_t* stamp;   // [4][Spad] last_recv_time per handle, ms of the caller's clock (kLvUnstamped: no poll yet)
  uint8_t* flags;   // [4][Spad] kLvNotifySent | kLvEventSent per handle
  uint32_t* ev_n;   // [Spad] events since enable or restart
  int32_t* ev;      // [LV_EV_ROWS][kLvEvents][Spad] the newest events' kind, handle, value (slot: count % kLvEvents)
  int32_t timeout_ms, notify_ms;  // disconnect_timeout, disconnect_notify_start (builder.rs:175-184)
};

// P2PSession::disconnect_player_at_frame(h, local_connect_status[h].last_frame)
// (p2p_session.rs:555-581) on the packed bookkeeping rows of session s: the handle's disconnected
// flag, and the resimulation from last_frame + 1 when the session is past it.
__device__ inline void p2p_disconnect_write(int32_t* qs, size_t sp, int s, int h) {
  auto row = [&](int field) -> int32_t& { return qs[(QS_PLAYER0 + field * 4 + h) * sp + s]; };
  const int32_t cur = qs[QS_CUR * sp + s];
  const uint32_t m = static_cast<uint32_t>(row(QF_MISC));
  const int32_t last = (m & kQmEsc) ? row(QF_ABS0 + 1) : fd_dec(static_cast<uint32_t>(row(QF_LA_CONN)) >> 16, cur);
  row(QF_MISC) = static_cast<int32_t>(m | kQmDisc);
  if (cur > last) qs[QS_DISC_FRAME * sp + s] = last + 1;
}

// The timer half of one poll_remote_clients (p2p_session.rs:375-415), one lane per session over its
// remote handles in ascending order, so a session's event ring has one writer.  Everything whose
// address is known up front (status, the caller's bytes, flags, stamps, the event count) is loaded
// before the first store.  The bookkeeping rows are read only where they decide something: the
// handle's disconnected flag by a lane whose step raises an event (a disconnected handle's endpoint
// no longer runs, :396-401: it stamps and raises nothing) or that owes state_out its bit 2, the
// rest by p2p_disconnect_write behind a Disconnected.  A healthy endpoint stores its stamp; one
// with nothing received and no timer due stores nothing.
//   received, requested, state_out: uint8 [P][S]; requested and state_out may be null.
template <int P>
__global__ void __launch_bounds__(256)
p2p_liveness_kernel(const LivenessParams lv, int32_t* __restrict__ qs, const int32_t* __restrict__ status,
                    const uint8_t* __restrict__ received, const uint8_t* __restrict__ requested,
                    uint8_t* __restrict__ state_out, int64_t now, uint32_t local_mask, int S, int Spad) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const size_t sp = static_cast<size_t>(Spad);
  const int32_t st = status[s];
  int64_t stamp[P];
  uint32_t flags[P], misc[P];
  bool rc[P], rq[P];
#pragma unroll
  for (int h = 0; h < P; ++h) {
    stamp[h] = kLvUnstamped;
    flags[h] = misc[h] = 0u;
    rc[h] = rq[h] = false;
    if ((local_mask >> h) & 1u) continue;
    const size_t o = static_cast<size_t>(h) * sp + s, c = static_cast<size_t>(h) * S + s;
    stamp[h] = lv.stamp[o];
    flags[h] = lv.flags[o];
    rc[h] = received[c] != 0;
    rq[h] = requested && requested[c] != 0;
    if (state_out) misc[h] = static_cast<uint32_t>(qs[(QS_PLAYER0 + QF_MISC * 4 + h) * sp + s]);
  }
  const uint32_t n0 = lv.ev_n[s];
  uint32_t n = n0;
  const bool dead = st == kP2PStatusPanic;  // a panicked session is skipped entirely
#pragma unroll
  for (int h = 0; h < P; ++h) {
    const size_t c = static_cast<size_t>(h) * S + s;
    if ((local_mask >> h) & 1u) {
      if (state_out) state_out[c] = 0;
      continue;
    }
    uint32_t fl = flags[h];
    bool disc = (misc[h] & kQmDisc) != 0;
    if (!dead) {
      const size_t o = static_cast<size_t>(h) * sp + s;
      const LivenessStep r = liveness_step(stamp[h], fl, rc[h], rq[h], now, lv.notify_ms, lv.timeout_ms);
      if (r.stamp != stamp[h]) lv.stamp[o] = r.stamp;
      if (r.events) {
        if (!state_out) disc = (static_cast<uint32_t>(qs[(QS_PLAYER0 + QF_MISC * 4 + h) * sp + s]) & kQmDisc) != 0;
        if (!disc) {
          fl = r.flags;
          lv.flags[o] = static_cast<uint8_t>(fl);
#pragma unroll
          for (int k = 0; k < kLvSlots; ++k) {
            if (!((r.events >> k) & 1u)) continue;
            const size_t q = static_cast<size_t>(n % kLvEvents) * sp + s, plane = static_cast<size_t>(kLvEvents) * sp;
            const int32_t kind = liveness_event_kind(k);
            lv.ev[LV_EV_KIND * plane + q] = kind;
            lv.ev[LV_EV_HANDLE * plane + q] = h;
            lv.ev[LV_EV_VALUE * plane + q] = kind == kLvInterrupted ? r.value : 0;
            n += 1u;
          }
          if (r.events & (kLvEvRequested | kLvEvTimedOut)) {  // handle_event's Event::Disconnected (p2p_session.rs:835-847)
            p2p_disconnect_write(qs, sp, s, h);
            disc = true;
          }
        }
      }
    }
    if (state_out) state_out[c] = static_cast<uint8_t>(fl | (disc ? 4u : 0u));
  }
  if (n != n0) lv.ev_n[s] = n;
}

}  // namespace rb
