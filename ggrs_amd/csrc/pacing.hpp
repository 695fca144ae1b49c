// ggrs_amd/csrc/pacing.hpp — per-session pacing of P2P batches
// (include/ggrs_amd.h rb_p2p_run_ticks_paced, rb_p2p_pace): the caller's frame
// loop of ex_game_p2p.rs:80-122, where poll_remote_clients runs on every
// iteration and add_local_input / advance_frame only when the session's own
// accumulator says a frame is due, and a session that is ahead stretches its
// frame time by 10%.
//
// p2p_kernel is not touched: a session whose status word is kP2PStatusPanic
// returns from it before any store, so a paced tick hands it a *view* of the
// status array in which every parked session reads as panicked
// (p2p_poll_kernel builds it), and copies the view back for the running
// sessions afterwards (p2p_unpark_kernel).  What a parked session still owes
// the tick, poll_remote_clients, p2p_poll_kernel does on the packed
// bookkeeping rows and the HBM input ring.  Both kernels are independent of
// the game: templated on input bytes and player count only.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "p2p.hpp"
#include "time_sync.hpp"

namespace rb {

// the pacer's integer frame time (ex_game_p2p.rs:91-104 at the nominal rate): a tick is worth
// kPaceTick, a frame costs kPaceTick, or 10% more while the session is ahead (fps_delta *= 1.1)
constexpr int32_t kPaceTick = 10, kPaceAhead = 11;

struct PaceParams {
  int32_t* view;      // [Spad] the status array p2p_kernel sees in a paced tick
  uint32_t* parked;   // [Spad] parked ticks per session since create
  int32_t* acc;       // [Spad] the pacer's accumulator
};

// q_add's input classes are the fan-out's (q.mtf); never read here
struct PollNoCanon {
  __host__ __device__ static constexpr uint32_t apply(uint32_t v) { return v; }
};

// The first launch of a paced tick, one thread per session: the status view, and for a parked
// session that has not panicked poll_remote_clients (p2p_session.rs:375-415) and nothing else:
//   - update_local_frame_advantage of every running endpoint (:387-392; time sync on only), the
//     arithmetic of p2p_time_sync_kernel;
//   - Event::Input in frame order for every remote, connected handle (handle_event, :838-852):
//     the poll loop of p2p_kernel's tick_begin on the packed rows (q_unpack / q_pack, escape rows
//     included) and the HBM input ring;
//   - input_queue.rs:181's assert fired during the poll: the session panics (the real status
//     word, counters[2]) exactly as a running tick's poll does.
// ts.state == nullptr: time sync off.
template <int IB, int P>
__global__ void __launch_bounds__(256)
p2p_poll_kernel(const PaceParams pc, const uint8_t* __restrict__ run_mask, int32_t* __restrict__ qs, uint8_t* __restrict__ ring,
                int32_t* __restrict__ status, uint32_t* __restrict__ counters, const int32_t* __restrict__ upto,
                const uint8_t* __restrict__ remote_in, int32_t remote_frames, int32_t remote_mask, int32_t remote_delay, uint32_t local_mask,
                const TimeSyncParams ts, int S, int Spad) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const size_t sp = static_cast<size_t>(Spad);
  const bool run = run_mask[s] != 0;
  const int32_t st = status[s];
  pc.view[s] = run ? st : kP2PStatusPanic;
  if (run) return;
  pc.parked[s] += 1u;
  if (st == kP2PStatusPanic) return;
  const int32_t cur = qs[QS_CUR * sp + s];
  const RingIO<IB> io{ring, P, Spad};
  const uint32_t rstride = static_cast<uint32_t>(P) * static_cast<uint32_t>(S) * IB;
  bool ovf = false;
#pragma unroll
  for (int h = 0; h < P; ++h) {
    if ((local_mask >> h) & 1u) continue;
    auto qrow = [&](int field) -> int32_t& { return qs[(QS_PLAYER0 + field * 4 + h) * sp + s]; };
    uint32_t w[4];
    int32_t ab[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = static_cast<uint32_t>(qrow(QF_LA_CONN + i));
    if (w[3] & kQmEsc) {
#pragma unroll
      for (int i = 0; i < 7; ++i) ab[i] = qrow(QF_ABS0 + i);
    }
    const QFields f = q_unpack(w, cur, ab);
    if (f.disc) continue;  // handle_event ignores a disconnected player (:852); its endpoint no longer runs
    const int32_t end = min(upto[static_cast<size_t>(h) * S + s], remote_frames - 1);
    if (ts.state && end != kNullFrame) {
      const int32_t ping = ts.state[static_cast<size_t>(TS_RTT + h) * sp + s] / 2;
      ts.state[static_cast<size_t>(TS_LOCAL_ADV + h) * sp + s] = end + (ping * ts.fps) / 1000 - cur;
    }
    DevQueue q{};
    q.last_added = f.la;
    q.conn_last = f.conn;
    q.pred_frame = f.pred;
    q.first_inc = f.fi;
    q.last_req = f.req;
    q.tail = f.tail;
    q.len = f.len;
    q.disc = false;
    q.pred_val = IB == 1 ? f.pv : static_cast<uint32_t>(qrow(QF_PRED_VAL));
    const uint8_t* const rbase = remote_in + (static_cast<size_t>(h) * S + s) * IB;
    int32_t fr = q.conn_last == kNullFrame ? remote_delay : q.conn_last + 1;
    if (fr > end) continue;  // nothing new: the rows stay as they are
    for (; fr <= end; ++fr) {
      const uint8_t* src = rbase + static_cast<uint64_t>(static_cast<uint32_t>(max(fr, 0) & remote_mask)) * rstride;
      const uint32_t v = IB == 4 ? *reinterpret_cast<const uint32_t*>(src) : *src;
      q_add<PollNoCanon>(q, io, h, static_cast<unsigned>(s), fr, v);  // add_remote_input (frame delay 0)
      q.conn_last = fr;
    }
    ovf |= q_overflow(q);
    const QFields g{q.last_added, q.conn_last, q.pred_frame, q.first_inc, q.last_req, q.tail, q.len, false, f.pv};
    const QPacked pk = q_pack(g, cur);
#pragma unroll
    for (int i = 0; i < 4; ++i) qrow(QF_LA_CONN + i) = static_cast<int32_t>(pk.w[i]);
    if (pk.esc) {
      const int32_t a2[7] = {g.la, g.conn, g.pred, g.fi, g.req, g.tail, g.len};
#pragma unroll
      for (int i = 0; i < 7; ++i) qrow(QF_ABS0 + i) = a2[i];
    }
  }
  if (ovf) {
    status[s] = kP2PStatusPanic;
    atomicAdd(&counters[2], 1u);
  }
}

// The last launch of a paced tick: what p2p_kernel left in the view becomes the status of the
// sessions that ran.  The real status array never holds a parked session's fake panic.
__global__ void p2p_unpark_kernel(const int32_t* __restrict__ view, const uint8_t* __restrict__ run_mask,
                                  int32_t* __restrict__ status, int S) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S || !run_mask[s]) return;
  const int32_t v = view[s];
  if (status[s] != v) status[s] = v;
}

// One step of the pacer, acc starting at 0: the next tick's run-mask byte.
__host__ __device__ inline bool pace_step(int32_t& acc, int32_t frames_ahead) {
  acc += kPaceTick;
  const int32_t cost = frames_ahead > 0 ? kPaceAhead : kPaceTick;
  const bool run = acc >= cost;
  if (run) acc -= cost;
  return run;
}

// frames_ahead -> the next tick's run mask, on the device (rb_p2p_pace).  A panicked session runs:
// it returns early from the tick anyway.
__global__ void p2p_pace_kernel(const PaceParams pc, const int32_t* __restrict__ ts_state, const int32_t* __restrict__ status,
                                uint8_t* __restrict__ run_mask, int S, int Spad) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  int32_t acc = pc.acc[s];
  const bool run = pace_step(acc, ts_state[static_cast<size_t>(TS_FRAMES_AHEAD) * Spad + s]);
  pc.acc[s] = acc;
  run_mask[s] = (run || status[s] == kP2PStatusPanic) ? 1 : 0;
}

}  // namespace rb
