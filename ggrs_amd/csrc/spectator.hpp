// ggrs_amd/csrc/spectator.hpp — device side of batched SpectatorSession
// (sessions/p2p_spectator_session.rs:109-139 advance_frame, :173-202
// inputs_at_frame, :233-246 Event::Input).
//
// S independent spectators, each a rollback-free replica of one host session:
// it advances only on the inputs the host has confirmed and sent
// (P2PSession::send_confirmed_inputs_to_spectators, p2p_session.rs:676-703;
// here rb_p2p_export_confirmed_inputs), one frame per tick, or catchup_speed
// frames while it is more than max_frames_behind behind.  The network layer is
// the caller's, as for the P2P batches: per tick it passes the newest frame
// the host's Input messages have delivered (`upto`) and the inputs by frame.
//
// The 60-slot input ring (SPECTATOR_BUFFER_SIZE, :16, :28, :59-62) stays
// implicit.  The host sends every confirmed frame in order from frame 0
// (next_spectator_frame, p2p_session.rs:201, :681-702), so after deliveries up
// to last_recv, slot f % 60 holds the newest frame <= last_recv congruent to f
// (or the blank NULL_FRAME input).  inputs_at_frame (:177-187) compares that
// slot's frame tag with f:
//   tag < f  (PredictionThreshold)      exactly when last_recv < f
//   tag > f  (SpectatorTooFarBehind)    exactly when last_recv >= f + 60
// and otherwise the slot holds frame f itself.  So the kernel decides by
// last_recv alone and reads frame f from the caller's by-frame tensor in place.
//
// Both errors can only occur on a tick's first frame.  A tick takes more than
// one frame only when behind = last_recv - current > max_frames_behind, and
// the validated configuration (builder.rs:210-244, rb_spectator_create) gives
// catchup_speed < max_frames_behind < 60.  So all of its frames
// current + 1 .. current + catchup_speed are <= last_recv (no
// PredictionThreshold), and last_recv >= f + 60 for a later frame f implies it
// for the first one.  The reference's path in which current_frame has moved
// but the requests are dropped (:125-136, the `?` after earlier iterations) is
// therefore unreachable, and it is not built: a tick either advances all of its
// frames or none.
//
// Device layout (Spad = S rounded up to 64; L = G::kLanes lanes per session,
// the layout of the P2P batches, p2p.hpp):
//   live    [NW planes][Spad*L]  game state after frame `current` (its frame word is current + 1)
//   cs      [Spad] CS            G::checksum(state, current + 1): what the host's cell of that frame holds
//   frames  [2][Spad] i32        current_frame, last_recv_frame (both start at NULL_FRAME, :67-68)
//   status  [2][Spad] i32        the last tick's rb_status and AdvanceFrame count
//   host    [2][4][Spad] i32     host_connect_status: last_frame, disconnected (:29, :243-245)
//   stats   [3][Spad] u64        AdvanceFrames, PredictionThreshold ticks, TooFarBehind ticks
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "games.hpp"

namespace rb {

constexpr int32_t kSpectatorBuffer = 60;  // SPECTATOR_BUFFER_SIZE (p2p_spectator_session.rs:16)
constexpr int32_t kSpectatorOk = 0, kSpectatorThreshold = 1, kSpectatorTooFar = 5;  // rb_status values
enum : int { SPT_ADV = 0, SPT_THRESHOLD = 1, SPT_TOO_FAR = 2, SPT_COUNT = 3 };

struct SpectatorParams {
  uint32_t* live;
  void* cs;
  int32_t* frames;
  int32_t* status;
  const int32_t* host_last;  // [4][Spad]
  const int32_t* host_disc;  // [4][Spad] 0 / 1
  unsigned long long* stats;
  uint32_t* counters;        // [1]: unexpected math paths (the games' advance reports them)
  const int32_t* upto;       // tick t: upto[t * S + s], the newest frame delivered before the tick
  const uint8_t* in;         // frame f, player h: in + (((f & in_mask) * P + h) * S + s) * IB
  // linear tensor: the frames it holds (a delivery mark past them counts as in_frames - 1); a
  // delivery ring (rb_spectator_set_delivery_ring): INT32_MAX, no frame is clamped
  int32_t in_frames;
  int32_t S, Spad, T;
  int32_t max_behind, catchup;  // 1 <= catchup < max_behind < kSpectatorBuffer
  // linear: all ones below the sign bit; a delivery ring of R frames: R - 1, frame f in slot
  // f & in_mask.  The last field: a plug-in built before it reads the fields above where they were.
  int32_t in_mask;
};
static_assert(offsetof(SpectatorParams, in_frames) == 80 && offsetof(SpectatorParams, S) == 84 &&
                  offsetof(SpectatorParams, catchup) == 100 && offsetof(SpectatorParams, in_mask) == 104,
              "SpectatorParams changed layout: bump RB_PLUGIN_ABI (include/ggrs_amd_game.hpp)");

// One launch = T ticks of SpectatorSession::advance_frame for every session.
// The game words stay in registers across the ticks.  Catch-up differs per
// session: a tick's frame loop runs to the wave's largest frame count with the
// other sessions masked.  The input of frame current + 1 is always in flight
// one frame ahead (its address depends on nothing but `current`), so a frame's
// AdvanceFrame does not start with a global-memory round trip.
template <class G>
__global__ void __launch_bounds__(256) spectator_kernel(const SpectatorParams p) {
  using InRec = typename G::InRec;
  using CS = typename G::CS;
  constexpr int NW = G::NWL, L = G::kLanes, P = G::kPlayers, IB = G::kInputBytes;
  constexpr bool kSplit = L > 1;  // lane h of the group owns player h
  constexpr int PPL = kSplit ? 1 : P;
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned s = g / L;
  const int lane = static_cast<int>(g % L);
  if (s >= static_cast<unsigned>(p.S)) return;  // whole lane groups leave together
  const unsigned Spad = static_cast<unsigned>(p.Spad), Gpad = Spad * L;
  auto player_of = [&](int j) __attribute__((always_inline)) { return kSplit ? lane : j; };

  uint32_t w[NW];
  load_words<NW>(p.live, static_cast<int>(Gpad), static_cast<int>(g), w);
  int32_t cur = p.frames[s], recv = p.frames[Spad + s];
  // host_connect_status of this lane's players; a lane without a player (P = 3 in a 4-lane group,
  // the brawler's lanes past P) reads player P - 1's and uses nothing of it
  int32_t hlast[PPL];
  bool hdisc[PPL];
  const uint8_t* ibase[PPL];
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    const int h = min(player_of(j), P - 1);
    hlast[j] = p.host_last[static_cast<unsigned>(h) * Spad + s];
    hdisc[j] = p.host_disc[static_cast<unsigned>(h) * Spad + s] != 0;
    ibase[j] = p.in + (static_cast<size_t>(h) * p.S + s) * IB;
  }
  // in[frame][P][S]: a per-lane base and a 32-bit frame stride (P * S * IB < 2^32, rb_spectator_run_ticks)
  const uint32_t istride = static_cast<uint32_t>(P) * static_cast<uint32_t>(p.S) * IB;
  const int32_t last_in = p.in_frames - 1;
  auto load_in = [&](int j, int32_t f) __attribute__((always_inline)) -> uint32_t {
    f = max(0, min(f, last_in)) & p.in_mask;  // always a valid address; a frame past last_recv is loaded and never used
    const uint8_t* src = ibase[j] + static_cast<uint64_t>(static_cast<uint32_t>(f)) * istride;
    return IB == 4 ? *reinterpret_cast<const uint32_t*>(src) : *src;
  };
  uint32_t vin[PPL];  // the inputs of frame cur + 1
#pragma unroll
  for (int j = 0; j < PPL; ++j) vin[j] = load_in(j, cur + 1);
  int32_t up = p.upto[s];

  int32_t status = kSpectatorOk, nadv = 0;  // of the last tick (T >= 1)
  uint32_t tot_adv = 0, tot_thr = 0, tot_far = 0;
  for (int t = 0; t < p.T; ++t) {
    // Event::Input (:233-237): the deliveries are in order, last_recv_frame only grows
    recv = max(recv, min(up, last_in));
    up = p.upto[static_cast<size_t>(min(t + 1, p.T - 1)) * p.S + s];  // the next tick's, one tick ahead
    // frames_to_advance (:119-123)
    const int32_t n = (recv - cur > p.max_behind) ? p.catchup : 1;
    // inputs_at_frame (:177-187) of the tick's first frame, by the implicit ring (above); the later
    // frames of a catch-up tick cannot fail
    const int32_t f0 = cur + 1;
    status = recv < f0 ? kSpectatorThreshold : (recv >= f0 + kSpectatorBuffer ? kSpectatorTooFar : kSpectatorOk);
    nadv = status == kSpectatorOk ? n : 0;
    tot_thr += status == kSpectatorThreshold ? 1u : 0u;
    tot_far += status == kSpectatorTooFar ? 1u : 0u;
    for (int32_t k = 0; __ballot(k < nadv) != 0ull; ++k) {
      if (k < nadv) {
        const int32_t f = cur + 1;
        uint64_t rec = 0;
        uint32_t dmask = 0u;
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
          const int h = player_of(j);
          if (h >= P) continue;
          // (:193-199) a player the host reports disconnected before f: the host sent a blank input
          // (sync_layer.rs:210-211); the status is Disconnected
          if (hdisc[j] && hlast[j] < f) dmask |= 1u << h;
          else rec |= static_cast<uint64_t>(vin[j]) << (8 * IB * h);
        }
#pragma unroll
        for (int j = 0; j < PPL; ++j) vin[j] = load_in(j, f + 1);
        advance_frame<G>(w, static_cast<InRec>(rec), lane, dmask, p.counters);
        cur = f;
      }
    }
    tot_adv += static_cast<uint32_t>(nadv);
  }

  // the checksum the host stored in its cell of frame cur + 1 (SaveGameState{frame}, sync_layer.rs:118-125)
  const CsCtx ctx{0ull, s, 0u};
  const CS c = G::checksum(w, cur + 1, lane, ctx);
  store_words<NW>(p.live, static_cast<int>(Gpad), static_cast<int>(g), w);
  if (lane == 0) {
    reinterpret_cast<CS*>(p.cs)[s] = c;
    p.frames[s] = cur;
    p.frames[Spad + s] = recv;
    p.status[s] = status;
    p.status[Spad + s] = nadv;
  }
  // The totals as rb_p2p_totals keeps them (p2p.hpp): return-less atomics, a full wave's counts
  // summed first and added at its first session's column; only the sums are read.
  const bool lead = lane == 0;
  if (__ballot(1) == ~0ull) {
    uint32_t cnt[SPT_COUNT] = {lead ? tot_adv : 0u, lead ? tot_thr : 0u, lead ? tot_far : 0u};
#pragma unroll
    for (int i = 0; i < SPT_COUNT; ++i)
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) cnt[i] += static_cast<uint32_t>(__shfl_xor(static_cast<int>(cnt[i]), o, 64));
    if ((g & 63u) == 0) {
#pragma unroll
      for (int i = 0; i < SPT_COUNT; ++i)
        if (cnt[i]) atomicAdd(&p.stats[static_cast<unsigned>(i) * Spad + s], static_cast<unsigned long long>(cnt[i]));
    }
  } else if (lead) {
    if (tot_adv) atomicAdd(&p.stats[SPT_ADV * Spad + s], static_cast<unsigned long long>(tot_adv));
    if (tot_thr) atomicAdd(&p.stats[SPT_THRESHOLD * Spad + s], static_cast<unsigned long long>(tot_thr));
    if (tot_far) atomicAdd(&p.stats[SPT_TOO_FAR * Spad + s], static_cast<unsigned long long>(tot_far));
  }
}

}  // namespace rb
