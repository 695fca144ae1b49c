// ggrs_amd/csrc/p2p_engine.hip — host side of the P2PSession batches
// (include/ggrs_amd.h rb_p2p_*): buffers, validation (builder.rs), launches of
// p2p_kernel (p2p.hpp) and the read-backs the parity tests use.
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "liveness.hpp"
#include "pacing.hpp"
#define RB_RESTART_DEFINE  // restart_kernel and the move kernels live in this translation unit
#include "migrate.hpp"
#include "time_sync.hpp"

using namespace rb;

struct rb_p2p {
  rb_p2p_config cfg{};
  std::unique_ptr<GameOps> ops;
  int S = 0, Spad = 0, W = 0, P = 0, block = 256;
  int device = 0;
  uint32_t simds = 1024;  // SIMDs of the device (MI355X: 256 CUs x 4)
  hipStream_t own_stream = nullptr, stream = nullptr;
  uint32_t* snap = nullptr;
  void* cs = nullptr;
  int32_t* tag = nullptr;
  void* ring = nullptr;
  uint32_t* live = nullptr;
  int32_t* qs = nullptr;
  int32_t* status = nullptr;
  int32_t* trace = nullptr;
  uint32_t* counters = nullptr;
  unsigned long long* stats = nullptr;  // [ST_COUNT][Spad]
  bool fanout = false;
  bool per_player = false;   // RB_P2P_FLAG_FANOUT_PER_PLAYER
  bool sync_ticks = false;   // RB_P2P_SYNC_TICKS=1 at create: lock-step ticks (p2p.hpp kAsync off)
  bool fan_generic = false;  // RB_FANOUT_GENERIC=1 at create: fanout_kernel for every game
  uint32_t* spec_state = nullptr;
  uint32_t* spec_cells = nullptr;
  void* spec_cs = nullptr;
  int32_t* spec_meta = nullptr;
  std::vector<uint8_t> disconnected;  // host mirror [P][S] of ConnectionStatus::disconnected (validation)
  uint8_t* disc_mask = nullptr;       // [S] device copy of rb_p2p_disconnect_player's session mask
  uint32_t* tmpl = nullptr;           // the fresh columns restart_kernel copies (restart.hpp PlaneSet::tmpl), from create
  std::vector<uint32_t> tmpl_host;
  RestartIndex restart_idx;           // rb_p2p_restart_sessions' selected sessions
  RestartIndex move_idx;              // rb_p2p_export_sessions' / rb_p2p_import_sessions' (a restart in flight keeps its own slots)
  uint32_t* refused = nullptr;        // [1] records rb_p2p_import_sessions refused since create (made by the first import)
  bool mirror_stale = false;          // an import wrote qs: `disconnected` is refreshed from it before its next use
  DesyncParams ds{};                  // desync detection buffers (desync_interval > 0)
  PeerParams peer{};                  // peers' connect-status reports (RB_P2P_FLAG_PEER_STATUS)
  int32_t* exp_state = nullptr;       // [2][Spad]: next_spectator_frame, export status (rb_p2p_export_confirmed_inputs)
  TimeSyncParams ts{};                // rb_p2p_time_sync_enable: the per-session rows and windows (time_sync.hpp)
  bool ts_on = false;
  int32_t* ts_log = nullptr;          // [ts_log_ticks][kTlRows][Spad] the tick log, every kTlEnd row unwritten between calls
  int32_t ts_log_ticks = 0;
  PaceParams pace{};                  // rb_p2p_run_ticks_paced / rb_p2p_pace: the status view, parked ticks, the pacer's accumulator
  bool ticked = false;                // a tick has run (rb_p2p_time_sync_enable comes before the first)
  LivenessParams lv{};                // rb_p2p_liveness_enable: stamps, flags, the event ring and the two delays (liveness.hpp)
  bool lv_on = false;
  int64_t lv_now = 0;                 // the newest now_ms a poll has passed
  int32_t ring_frames = 0;            // rb_p2p_set_delivery_ring: R, or 0 for linear by-frame tensors (host state only)
  DeviceOwner res;                    // every device buffer, pinned buffer and event of the batch
  bool prof = false;
  EventPool prof_ev{res};
  LaunchClock clock;  // rb_p2p_launch_clock_arm
  // the adaptive fan-out (RB_P2P_FLAG_FANOUT without _ALWAYS, include/ggrs_amd.h)
  struct FanPolicy {
    bool adaptive = false;
    bool active = true;          // presimulating
    bool open = false;           // a measurement window is open (its start sums are in host[0..1])
    bool pending = false;        // its end sums are on their way to host[2..3] (event `ev`)
    int32_t ticks = 0;           // ticks into the window (active) or into the pause (inactive)
    int32_t since_end = 0;       // ticks since the pending window ended (the decision waits kFanDecideTicks)
    uint32_t min_permille = 150;
    unsigned long long* dev = nullptr;   // [4] device sums: selects, loads (window start; end)
    unsigned long long* host = nullptr;  // [4] pinned copies
    hipEvent_t ev = nullptr;
    double last_frac = -1.0;
    int32_t windows = 0, turned_off = 0;
  } fan;
  std::string last_err;

  // what migrate.hpp's restart and move need of a batch
  static constexpr const char* kApi = "rb_p2p";
  void planes(PlaneSet& ps);
  std::vector<uint32_t> record_config() const;
  rb_status before_move();
  ~rb_p2p() {
    if (!own_stream) return;  // nothing was made
    DeviceScope dev_scope(device);
    (void)hipStreamSynchronize(stream);
    res.release_all();
    (void)hipStreamDestroy(own_stream);
  }
};
constexpr int32_t kFanProbeTicks = 64, kFanPauseTicks = 960;
constexpr uint64_t kFanMinRollbacks = 64;  // a window with fewer rollbacks decides nothing

namespace {
// The adaptive fan-out's measurement: selects and LoadGameStates summed over the batch into out[0..1].
__global__ void fan_sums_kernel(const unsigned long long* __restrict__ stats, int S, int Spad,
                                unsigned long long* __restrict__ out) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long sel = s < S ? stats[static_cast<size_t>(ST_SELECT) * Spad + s] : 0ull;
  unsigned long long ld = s < S ? stats[static_cast<size_t>(ST_LOAD) * Spad + s] : 0ull;
  for (int o = 32; o > 0; o >>= 1) {
    sel += __shfl_down(sel, o, 64);
    ld += __shfl_down(ld, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&out[0], sel);
    atomicAdd(&out[1], ld);
  }
}

__global__ void p2p_disconnect_kernel(int32_t* qs, const uint8_t* mask, int32_t S, int32_t Spad, int32_t h) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S || (mask && !mask[s])) return;
  p2p_disconnect_write(qs, static_cast<size_t>(Spad), s, h);
}

// UdpProtocol::on_checksum_report (protocol.rs:710-722) for the endpoint of
// remote handle h in every session: the peer's reports, oldest first,
// in[k * S + s] for k < K (frame NULL_FRAME = none).
__global__ void p2p_receive_reports_kernel(DesyncParams d, const rb_checksum_report* __restrict__ in, int K, int S,
                                           int Spad, int h) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  auto at = [&](size_t k) { return k * static_cast<size_t>(Spad) + static_cast<size_t>(s); };
  const size_t m = static_cast<size_t>(h) * 3;
  int head = d.rh_meta[at(m)], n = d.rh_meta[at(m + 1)], last = d.rh_meta[at(m + 2)];
  for (int k = 0; k < K; ++k) {
    const rb_checksum_report r = in[static_cast<size_t>(k) * S + s];
    if (r.frame == kNullFrame || !(last < r.frame)) continue;
    if (n > kMaxChecksumHistory) {  // retain(|&frame, _| frame > last_added - MAX): the oldest leave the front
      while (n > 0 && d.rh_frame[at(static_cast<size_t>(h) * kCsHist + static_cast<size_t>(head))] <= last - kMaxChecksumHistory) {
        head = (head + 1) % kCsHist;
        --n;
      }
    }
    last = r.frame;
    if (n >= kCsHist) continue;  // cannot happen: at most 33 entries
    const size_t slot = static_cast<size_t>(h) * kCsHist + static_cast<size_t>((head + n) % kCsHist);
    d.rh_frame[at(slot)] = r.frame;
    d.rh_lo[at(slot)] = r.checksum_lo;
    d.rh_hi[at(slot)] = r.checksum_hi;
    ++n;
  }
  d.rh_meta[at(m)] = head;
  d.rh_meta[at(m + 1)] = n;
  d.rh_meta[at(m + 2)] = last;
}

// The reports sent since the last take, oldest first, out[k * S + s] for
// k < kOutbox (only the newest kOutbox are kept); resets the outbox.
__global__ void p2p_take_reports_kernel(DesyncParams d, rb_checksum_report* __restrict__ out, int S, int Spad) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  auto at = [&](int k) { return static_cast<size_t>(k) * static_cast<size_t>(Spad) + static_cast<size_t>(s); };
  const uint32_t n = d.ob_n[s];
  const uint32_t cnt = n < static_cast<uint32_t>(kOutbox) ? n : static_cast<uint32_t>(kOutbox);
  for (int k = 0; k < kOutbox; ++k) {
    rb_checksum_report r{0, 0, kNullFrame, kNullFrame};
    if (static_cast<uint32_t>(k) < cnt) {
      const int q = static_cast<int>((n - cnt + static_cast<uint32_t>(k)) % kOutbox);
      r.frame = d.ob_frame[at(q)];
      r.checksum_lo = d.ob_cs[at(q)];
    }
    out[static_cast<size_t>(k) * S + s] = r;
  }
  d.ob_n[s] = 0;
}

// UdpProtocol::on_input's connect-status merge (protocol.rs:627-636) for one endpoint
__global__ void p2p_peer_status_kernel(PeerParams pp, const int32_t* __restrict__ last, const uint8_t* __restrict__ disc,
                                       int S, int Spad, int P, int e) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  for (int i = 0; i < P; ++i) {
    const size_t o = (static_cast<size_t>(e) * 4 + static_cast<size_t>(i)) * Spad + s;
    pp.last[o] = max(pp.last[o], last[static_cast<size_t>(i) * S + s]);
    pp.disc[o] = pp.disc[o] | (disc[static_cast<size_t>(i) * S + s] ? 1 : 0);
  }
}

// send_confirmed_inputs_to_spectators (p2p_session.rs:676-703) over confirmed_inputs
// (sync_layer.rs:203-217), one thread per session, on the bookkeeping rows and the input ring as the
// last launch left them (include/ggrs_amd.h rb_p2p_export_confirmed_inputs).
template <int IB>
__global__ void p2p_export_kernel(const int32_t* __restrict__ qs, const uint8_t* __restrict__ ring,
                                  const int32_t* __restrict__ status, int32_t* __restrict__ exp_state, int S, int Spad,
                                  int P, uint8_t* __restrict__ out, int32_t frames, int32_t ring_frames,
                                  int32_t* __restrict__ upto, int32_t* __restrict__ last_frames,
                                  uint8_t* __restrict__ disconnected) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const size_t sp = static_cast<size_t>(Spad);
  const int32_t cur = qs[QS_CUR * sp + s];
  int32_t conn[4];
  bool disc[4];
  int32_t confirmed = INT32_MAX, newest = kNullFrame;  // confirmed_frame (:487-498); the newest frame any queue holds
  for (int h = 0; h < P; ++h) {  // the packed rows, behind the escape bit the absolute ones (q_unpack)
    uint32_t w[4];
    int32_t ab[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) w[i] = static_cast<uint32_t>(qs[(QS_PLAYER0 + (QF_LA_CONN + i) * 4 + h) * sp + s]);
    if (w[3] & kQmEsc)
      for (int i = 0; i < 7; ++i) ab[i] = qs[(QS_PLAYER0 + (QF_ABS0 + i) * 4 + h) * sp + s];
    const QFields f = q_unpack(w, cur, ab);
    conn[h] = f.conn;
    disc[h] = f.disc;
    if (!f.disc) confirmed = min(confirmed, f.conn);
    newest = max(newest, f.la);
  }
  int32_t next = exp_state[s], est = exp_state[sp + s];
  // a slot the session still had to send was overwritten: frame `next` shares its slot with
  // next + 128.  Sticky, and a word of its own (the panic word and the ticks are untouched).
  if (newest != kNullFrame && newest - next >= kQueueLen) est = RB_P2P_EXPORT_OVERRUN;
  // linear: frames below `frames`; a delivery ring of R frames: frame `next` in slot next & (R - 1),
  // at most R frames a call (a slot is written once), the rest in the next call
  const int32_t mask = ring_frames ? ring_frames - 1 : INT32_MAX;
  const int32_t stop = !ring_frames ? frames : next > INT32_MAX - ring_frames ? INT32_MAX : next + ring_frames;
  if (est == RB_P2P_EXPORT_OK && status[s] != kP2PStatusPanic) {
    while (next <= confirmed && next < stop) {
      for (int h = 0; h < P; ++h) {
        const size_t src = (static_cast<size_t>(next & (kQueueLen - 1)) * P + h) * sp + s;
        const size_t dst = (static_cast<size_t>(next & mask) * P + h) * S + s;
        const bool blank = disc[h] && conn[h] < next;  // PlayerInput::blank_input (sync_layer.rs:210-211)
        if constexpr (IB == 4) reinterpret_cast<uint32_t*>(out)[dst] = blank ? 0u : reinterpret_cast<const uint32_t*>(ring)[src];
        else out[dst] = blank ? uint8_t{0} : ring[src];
      }
      ++next;
    }
  }
  exp_state[s] = next;
  exp_state[sp + s] = est;
  upto[s] = next - 1;  // RB_NULL_FRAME while nothing is exported
  for (int h = 0; h < P; ++h) {  // local_connect_status: the Input message's peer_connect_status
    last_frames[static_cast<size_t>(h) * S + s] = conn[h];
    disconnected[static_cast<size_t>(h) * S + s] = disc[h] ? 1 : 0;
  }
}

// UdpProtocol::send_input (protocol.rs:439-466) as P2PSession::add_local_input calls it for every
// remote endpoint (p2p_session.rs:330-353), in tensor form: one thread per session, the local
// handles' inputs of the frames after sent[h][s] up to local_connect_status[h].last_frame from the
// input ring into the caller's by-frame tensor (include/ggrs_amd.h rb_p2p_export_local_inputs).
// ring_frames: 0 for a linear tensor of `frames` frames, R for a delivery ring (frames == R), whose
// slot is the frame & (R - 1).
template <int IB>
__global__ void p2p_export_local_kernel(const int32_t* __restrict__ qs, const uint8_t* __restrict__ ring,
                                        const int32_t* __restrict__ status, int S, int Spad, int P, uint32_t local_mask,
                                        uint8_t* __restrict__ out, int32_t frames, int32_t ring_frames,
                                        int32_t* __restrict__ sent) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S || status[s] == kP2PStatusPanic) return;
  const size_t sp = static_cast<size_t>(Spad);
  const int32_t cur = qs[QS_CUR * sp + s];
  const int32_t mask = ring_frames ? ring_frames - 1 : INT32_MAX;
  for (int h = 0; h < P; ++h) {
    if (!((local_mask >> h) & 1u)) continue;
    uint32_t w[4];
    int32_t ab[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) w[i] = static_cast<uint32_t>(qs[(QS_PLAYER0 + (QF_LA_CONN + i) * 4 + h) * sp + s]);
    if (w[3] & kQmEsc)
      for (int i = 0; i < 7; ++i) ab[i] = qs[(QS_PLAYER0 + (QF_ABS0 + i) * 4 + h) * sp + s];
    const QFields f = q_unpack(w, cur, ab);
    // the newest frame the tensor can hold: all of them in a ring (its slots are reused)
    const int32_t last = ring_frames ? f.conn : min(f.conn, frames - 1);
    const int32_t done = sent[static_cast<size_t>(h) * S + s];
    if (last == kNullFrame || done >= last) continue;
    // the 128-entry input ring holds frames last_frame - 127 .. last_frame: older ones are lost
    // (the ring's R >= 128, so one call never writes a slot twice)
    int32_t fr = max(max(done, kNullFrame) + 1, f.conn - (kQueueLen - 1));
    if (fr > last) continue;  // (a linear tensor more than 127 frames short of last_frame)
    for (; fr <= last; ++fr) {
      const size_t src = (static_cast<size_t>(fr & (kQueueLen - 1)) * P + h) * sp + s;
      const size_t dst = (static_cast<size_t>(fr & mask) * P + h) * S + s;
      if constexpr (IB == 4) reinterpret_cast<uint32_t*>(out)[dst] = reinterpret_cast<const uint32_t*>(ring)[src];
      else out[dst] = ring[src];
    }
    sent[static_cast<size_t>(h) * S + s] = last;
  }
}

// session s's words [lanes][nw] from a block of lane planes, as its canonical image
void image_from_planes(const rb_p2p* b, const std::vector<uint32_t>& planes, int s, int32_t frame, uint8_t* out) {
  std::vector<uint32_t> w(static_cast<size_t>(b->ops->lanes) * b->ops->nw);
  session_words(planes.data(), b->ops->nw, b->ops->lanes, b->Spad, s, w.data());
  b->ops->image(w.data(), frame, out);
}
}  // namespace

namespace {
// ---- What a fresh session holds and the extent of each per-session buffer, one function per
// buffer group (restart.hpp).  The call that makes a group (make_group; create for the first four)
// allocates its buffers from these shapes and writes these values into every column,
// rb_p2p_restart_sessions into the selected sessions' columns: sizes and values stand here and
// nowhere else.  A group the batch does not have adds nothing.  Batch-wide buffers (counters,
// stats, the fan-out's sums) are not per session.

// SyncLayer::new, InputQueue::new and ConnectionStatus::default for every handle, no tick yet
void core_planes(rb_p2p* b, PlaneSet& ps) {
  const int NW = b->ops->nw, L = b->ops->lanes;
  std::vector<uint32_t> w0(static_cast<size_t>(L) * NW);
  b->ops->init_words(w0.data());
  ps.state(b->live, NW, L, 1, w0.data());  // State::new
  ps.state(b->snap, NW, L, b->W, nullptr);
  ps.fill(b->cs, b->ops->cs_bytes, b->W, 1, 0);
  ps.fill(b->tag, 4, b->W, 1, 0xff);  // GameState::default frame = NULL_FRAME
  ps.fill(b->ring, b->ops->input_bytes, static_cast<size_t>(kQueueLen) * b->P, 1, 0);  // blank inputs
  ps.fill(b->status, 4, 1, 1, 0);
  ps.fill(b->trace, 4, 1, 1, 0xff);  // no tick yet: NULL load frame (at frame 0), counts 0xFF
  // every frame NULL, current 0, connected, length 0, the first input at frame 0 (q_pack)
  std::vector<int32_t> qs(kQsFields, kNullFrame);
  const QPacked q0 = q_pack(QFields{kNullFrame, kNullFrame, kNullFrame, kNullFrame, kNullFrame, 0, 0, false, 0u}, 0);
  qs[QS_CUR] = 0;
  qs[QS_SAVED_CONF] = static_cast<int32_t>(fd_enc(kNullFrame, 0) | fd_enc(kNullFrame, 0) << 16);
  for (int h = 0; h < 4; ++h) {
    for (int i = 0; i < 4; ++i) qs[QS_PLAYER0 + (QF_LA_CONN + i) * 4 + h] = static_cast<int32_t>(q0.w[i]);
    qs[QS_PLAYER0 + QF_PRED_VAL * 4 + h] = 0;
    qs[QS_PLAYER0 + QF_MTF_N * 4 + h] = 0;  // the fan-out's candidate list starts empty
  }
  ps.row_values(b->qs, 1, qs);
}
// the fan-out: nothing valid yet.  The branch planes (spec_state, spec_cells, spec_cs) are read only
// behind a valid row, and a row is valid only for the tick after the launch that made it, unless
// the batch's adaptive policy has cleared it (fan_invalidate): batch-wide.  So a move carries
// neither: an imported session has no valid branch, as a restarted one.
void fanout_planes(rb_p2p* b, PlaneSet& ps) {
  if (!b->fanout) return;
  // branch columns per lane column: 16 (fanout_kernel: [session][branch][lane]; the one-player in-kernel
  // fan-out uses 16 + L of 16 * L), plus one own chain per lane for the per-player form
  const size_t K = kSpecBranches + (b->per_player ? 1 : 0), NW = b->ops->nw, W = b->W;
  ps.buffer(b->spec_state, 4, K * NW, b->ops->lanes);
  ps.buffer(b->spec_cells, 4, W * K * NW, b->ops->lanes);
  ps.buffer(b->spec_cs, b->ops->cs_bytes, W * K, 1);
  ps.fill(b->spec_meta, 4, SM_COUNT, 1, 0);
  ps.fresh_on_move();
}
// ConnectionStatus::default for every (endpoint, player)
void peer_planes(rb_p2p* b, PlaneSet& ps) {
  if (!b->peer.on) return;
  ps.fill(b->peer.last, 4, 16, 1, 0xff);  // NULL_FRAME
  ps.fill(b->peer.disc, 4, 16, 1, 0);
}
// empty histories, outbox and event rings (entries behind a count or a NULL frame are never read)
void desync_planes(rb_p2p* b, PlaneSet& ps) {
  DesyncParams& d = b->ds;
  if (d.interval <= 0) return;
  ps.fill(d.lh_frame, 4, kCsHist, 1, 0xff);  // NULL_FRAME: empty slot
  ps.fill(d.lh_cs, 8, kCsHist, 1, 0);
  ps.fill(d.rh_frame, 4, 4 * kCsHist, 1, 0xff);
  ps.row_values(d.rh_meta, 4, {0, 0, kNullFrame});  // head 0, length 0, last_added_checksum_frame NULL_FRAME
  ps.fill(d.ob_n, 4, 1, 1, 0);
  ps.fill(d.ev_n, 4, 1, 1, 0);
  ps.fill(d.ev_frame, 4, kEvents, 1, 0xff);
  ps.fill(d.ev_handle, 4, kEvents, 1, 0xff);
  // the entries behind those counts and frames: no fresh value, a move carries them
  ps.carried(d.rh_lo, 8, 4 * kCsHist, 1);
  ps.carried(d.rh_hi, 8, 4 * kCsHist, 1);
  ps.carried(d.ob_frame, 4, kOutbox, 1);
  ps.carried(d.ob_cs, 8, kOutbox, 1);
  ps.carried(d.ev_local, 8, kEvents, 1);
  ps.carried(d.ev_remote, 8, kEvents, 1);
}
// next_spectator_frame = 0 (p2p_session.rs:201), status RB_P2P_EXPORT_OK
void export_planes(rb_p2p* b, PlaneSet& ps) {
  if (b->exp_state || ps.make || ps.layout_only) ps.fill(b->exp_state, 4, 2, 1, 0);
}
// TimeSync::default, local / remote_frame_advantage 0, round_trip_time 0, next_recommended_sleep 0,
// frames_ahead 0, no event
void time_sync_planes(rb_p2p* b, PlaneSet& ps) {
  if (!b->ts_on && !ps.make) return;
  ps.fill(b->ts.state, 4, TS_ROWS, 1, 0);
  ps.fill(b->ts.win, 4, 2 * static_cast<size_t>(kTsWindow) * 4, 1, 0);
}
// nothing parked yet, acc = 0
void pace_planes(rb_p2p* b, PlaneSet& ps) {
  if (!b->pace.view && !ps.make && !(ps.layout_only && !b->fanout)) return;  // a fan-out batch never paces
  ps.fill(b->pace.view, 4, 1, 1, 0);
  ps.fill(b->pace.parked, 4, 1, 1, 0);
  ps.fill(b->pace.acc, 4, 1, 1, 0);
}
// every endpoint unstamped (its clock starts at its first poll), no flag, no event
void liveness_planes(rb_p2p* b, PlaneSet& ps) {
  if (!b->lv_on && !ps.make) return;
  ps.fill(b->lv.stamp, 8, 4, 1, 0xff);  // kLvUnstamped
  ps.fill(b->lv.flags, 1, 4, 1, 0);
  ps.fill(b->lv.ev_n, 4, 1, 1, 0);
  ps.carried(b->lv.ev, 4, static_cast<size_t>(LV_EV_ROWS) * kLvEvents, 1);  // the entries behind that count
}
// the groups create makes, the groups with templates first (their offsets are those of create)
void create_planes(rb_p2p* b, PlaneSet& ps) {
  core_planes(b, ps);
  desync_planes(b, ps);
  fanout_planes(b, ps);
  peer_planes(b, ps);
}
// Make a group: its buffers that do not exist yet, then its fresh values into every column, padding included.
rb_status make_group(rb_p2p* b, void (*group)(rb_p2p*, PlaneSet&)) {
  PlaneSet ps;
  ps.Spad = static_cast<size_t>(b->Spad);
  ps.make = &b->res;
  group(b, ps);
  RB_TRY(b, ps.err);
  ps.bind(b->tmpl);
  RB_TRY(b, restart_launch(ps, nullptr, static_cast<uint32_t>(b->Spad), b->stream));
  return RB_OK;
}
// The pacing buffers and the export's rows, made by the first call that needs them.
rb_status pace_reserve(rb_p2p* b) { return b->pace.view ? RB_OK : make_group(b, pace_planes); }
rb_status export_reserve(rb_p2p* b) { return b->exp_state ? RB_OK : make_group(b, export_planes); }
template <int IB>
auto poll_kernel_of(int P) {
  return P == 1 ? p2p_poll_kernel<IB, 1> : P == 2 ? p2p_poll_kernel<IB, 2> : P == 3 ? p2p_poll_kernel<IB, 3> : p2p_poll_kernel<IB, 4>;
}
}  // namespace

// every group the batch has
void rb_p2p::planes(PlaneSet& ps) {
  create_planes(this, ps);
  export_planes(this, ps);
  time_sync_planes(this, ps);
  pace_planes(this, ps);
  liveness_planes(this, ps);
}

extern "C" {

void rb_p2p_config_init(rb_p2p_config* c) {
  std::memset(c, 0, sizeof(*c));
  c->abi_version = RB_ABI_VERSION;
  c->game = RB_GAME_EX_GAME;
  c->num_sessions = 1;
  c->num_players = 2;     // builder.rs:13
  c->max_prediction = 8;  // builder.rs:20
  c->input_delay = 0;     // builder.rs:16
  c->device = 0;
  c->local_mask = 1u;     // handle 0 local, handle 1 remote (ex_game_p2p.rs's two-peer setup)
  c->remote_delay = 0;
  c->sparse_saving = 0;   // builder.rs:17 DEFAULT_SAVE_MODE
  c->fanout_candidates = kSpecBranches;
}

const char* rb_p2p_last_error(const rb_p2p* b) { return b ? b->last_err.c_str() : g_create_err.c_str(); }

rb_status rb_p2p_create(const rb_p2p_config* cfg, rb_p2p** out) {
  *out = nullptr;
  if (!cfg || cfg->abi_version != RB_ABI_VERSION) return fail(nullptr, RB_INVALID_REQUEST, "rb_p2p_config.abi_version mismatch");
  if (cfg->max_prediction <= 0)  // builder.rs:136-145
    return fail(nullptr, RB_INVALID_REQUEST, "Currently, only prediction windows above 0 are supported");
  if (cfg->num_players <= 0 || cfg->num_players > 4 || cfg->num_sessions <= 0 || cfg->input_delay < 0 ||
      cfg->remote_delay < 0 || cfg->desync_interval < 0)
    return fail(nullptr, RB_INVALID_REQUEST, "num_players must be 1..4; sizes and delays non-negative");
  const uint32_t all = (1u << cfg->num_players) - 1u;
  if ((cfg->local_mask & ~all) != 0)  // builder.rs:103-115: handles must be < num_players
    return fail(nullptr, RB_INVALID_REQUEST,
                "The player handle you provided is invalid. For a local player, the handle should be between 0 and num_players");
  if (cfg->local_mask == 0 || cfg->local_mask == all)
    return fail(nullptr, RB_INVALID_REQUEST, "a P2P batch needs at least one local and one remote handle");
  if (cfg->max_prediction > 64 || cfg->input_delay + cfg->max_prediction + 2 > kQueueLen)
    return fail(nullptr, RB_INVALID_REQUEST, "max_prediction / input delay do not fit the 128-entry input queue");
  if (cfg->game != RB_GAME_EX_GAME && cfg->game != RB_GAME_STUB && cfg->game != RB_GAME_STUB_ENUM &&
      cfg->game != RB_GAME_BRAWLER && cfg->game < RB_GAME_PLUGIN_BASE)
    return fail(nullptr, RB_INVALID_REQUEST,
                "P2P batches support ex_game, the stub games, the brawler and registered plugin games");
  auto ops = make_game(cfg->game, cfg->num_players, (cfg->flags & RB_FLAG_LANE_PER_SESSION) != 0);
  if (!ops) return fail(nullptr, RB_INVALID_REQUEST, "unsupported game / num_players combination (RB_FLAG_LANE_PER_SESSION: A/B builds only)");
  const bool fanout = (cfg->flags & RB_P2P_FLAG_FANOUT) != 0;
  if (fanout && (!ops->fanout_supported || cfg->sparse_saving))
    return fail(nullptr, RB_INVALID_REQUEST,
                "speculative fan-out needs ex_game with one lane per player or the brawler, no sparse saving");
  if (fanout && (cfg->fanout_candidates < 1 || cfg->fanout_candidates > kSpecBranches))
    return fail(nullptr, RB_INVALID_REQUEST, "fanout_candidates must be 1..16");
  const bool per_player = fanout && (cfg->flags & RB_P2P_FLAG_FANOUT_PER_PLAYER) != 0;
  if (per_player && (!ops->inlane_fanout || ops->input_alphabet > static_cast<uint32_t>(cfg->fanout_candidates)))
    return fail(nullptr, RB_INVALID_REQUEST,
                "per-player speculation needs independent players (ex_game) and fanout_candidates covering the "
                "input alphabet");
  if (static_cast<uint64_t>(cfg->max_prediction) * ops->nw * ops->lanes *
          ((static_cast<uint64_t>(cfg->num_sessions) + 63) / 64 * 64) >= (1ull << 32))
    return fail(nullptr, RB_INVALID_REQUEST, "batch too large for 32-bit snapshot offsets");
  // the fan-out's branch planes: a slot's offset is 64-bit (p2p.hpp), the words inside one slot
  // (planes x columns, load_words / store_words) are int offsets: at most 2^31 words per slot (the
  // brawler at 65,536 sessions is exactly that: 32 planes of 2^26 columns, the last plane's int
  // offset 31 x 2^26)
  if (fanout && static_cast<uint64_t>(ops->nw) * ops->lanes * (kSpecBranches + (per_player ? 1 : 0)) *
                        ((static_cast<uint64_t>(cfg->num_sessions) + 63) / 64 * 64) > (1ull << 31))
    return fail(nullptr, RB_INVALID_REQUEST, "batch too large for the fan-out's 31-bit branch-plane offsets");

  auto b = std::make_unique<rb_p2p>();
  b->cfg = *cfg;
  b->ops = std::move(ops);
  b->S = cfg->num_sessions;
  b->Spad = (cfg->num_sessions + 63) / 64 * 64;
  b->W = cfg->max_prediction;
  b->P = cfg->num_players;
  b->block = cfg->block_size ? static_cast<int>(cfg->block_size) : 256;
  if (b->block % 64 != 0 || b->block > 256) return fail(nullptr, RB_INVALID_REQUEST, "block_size must be 64, 128, 192 or 256");
  b->device = cfg->device;
  b->fanout = fanout;
  b->per_player = per_player;
  if (const char* e = std::getenv("RB_P2P_SYNC_TICKS")) b->sync_ticks = std::atoi(e) != 0;
  if (const char* e = std::getenv("RB_FANOUT_GENERIC")) b->fan_generic = std::atoi(e) != 0;
  b->fan.adaptive = fanout && (cfg->flags & RB_P2P_FLAG_FANOUT_ALWAYS) == 0;
  if (cfg->fanout_min_select_permille) b->fan.min_permille = cfg->fanout_min_select_permille;
  b->peer.on = (cfg->flags & RB_P2P_FLAG_PEER_STATUS) ? 1 : 0;
  b->ds.interval = cfg->desync_interval;
  b->disconnected.assign(static_cast<size_t>(b->P) * b->S, 0);
  // a failure from here on frees what was made (~rb_p2p) and leaves its message for rb_p2p_last_error(nullptr)
  DeviceScope dev_scope(b->device);
  int cus = 0;
  RB_TRY(nullptr, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
  b->simds = 4 * cus;  // 4 SIMDs per CU (CDNA)
  RB_TRY(nullptr, hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking));
  b->stream = b->own_stream;
  // the batch-wide buffers
  const size_t Sp = b->Spad;
  RB_TRY(nullptr, b->res.alloc(b->counters, 16));
  RB_TRY(nullptr, b->res.alloc(b->stats, ST_COUNT * Sp * 8));
  RB_TRY(nullptr, hipMemsetAsync(b->counters, 0, 16, b->stream));
  RB_TRY(nullptr, hipMemsetAsync(b->stats, 0, ST_COUNT * Sp * 8, b->stream));
  RB_TRY(nullptr, b->res.alloc(b->disc_mask, Sp));
  if (b->fan.adaptive) {
    RB_TRY(nullptr, b->res.alloc(b->fan.dev, 4 * sizeof(unsigned long long)));
    RB_TRY(nullptr, b->res.alloc_host(b->fan.host, 4 * sizeof(unsigned long long)));
    RB_TRY(nullptr, b->res.event(b->fan.ev, hipEventDisableTiming));
  }
  // every session fresh: the plane groups' buffers made, their values into every column, their
  // templates kept on the device for rb_p2p_restart_sessions
  PlaneSet ps;
  ps.Spad = Sp;
  ps.make = &b->res;
  create_planes(b.get(), ps);
  RB_TRY(nullptr, ps.err);
  b->tmpl_host = ps.tmpl;
  RB_TRY(nullptr, b->res.alloc(b->tmpl, ps.tmpl.size() * 4));
  RB_TRY(nullptr, hipMemcpyAsync(b->tmpl, ps.tmpl.data(), ps.tmpl.size() * 4, hipMemcpyHostToDevice, b->stream));
  ps.bind(b->tmpl);
  RB_TRY(nullptr, restart_launch(ps, nullptr, static_cast<uint32_t>(b->Spad), b->stream));
  RB_TRY(nullptr, hipStreamSynchronize(b->stream));
  *out = b.release();
  return RB_OK;
}

void rb_p2p_destroy(rb_p2p* b) { delete b; }

rb_status rb_p2p_set_stream(rb_p2p* b, void* s) {
  RB_TRY(b, hipStreamSynchronize(b->stream));
  b->stream = s ? static_cast<hipStream_t>(s) : b->own_stream;
  return RB_OK;
}

void* rb_p2p_get_stream(const rb_p2p* b) { return static_cast<void*>(b->stream); }

int32_t rb_p2p_state_bytes(const rb_p2p* b) { return b->ops->image_bytes; }
int32_t rb_p2p_input_bytes(const rb_p2p* b) { return b->ops->input_bytes; }

namespace {
// The batch's buffers and configuration for a P2P launch (the per-call tensors are the caller's).
P2PParams base_params(const rb_p2p* b) {
  P2PParams p{};
  p.snap = b->snap;
  p.cs = b->cs;
  p.tag = b->tag;
  p.ring = b->ring;
  p.live = b->live;
  p.qs = b->qs;
  p.status = b->status;
  p.trace = b->trace;
  p.counters = b->counters;
  p.stats = b->stats;
  p.S = b->S;
  p.Spad = b->Spad;
  p.W = b->W;
  p.delay = b->cfg.input_delay;
  p.remote_delay = b->cfg.remote_delay;
  p.local_mask = b->cfg.local_mask;
  p.sparse = b->cfg.sparse_saving != 0;
  p.sync_ticks = b->sync_ticks ? 1 : 0;
  p.many_waves = many_waves_per_simd(b->Spad, b->ops->lanes, b->simds) ? 1 : 0;
  p.fan_generic = b->fan_generic ? 1 : 0;
  p.fan_k = b->cfg.fanout_candidates;
  p.spec_on = b->fanout ? 1 : 0;
  p.spec_per_player = b->per_player && !b->fan_generic ? 1 : 0;
  p.spec_state = b->spec_state;
  p.spec_cells = b->spec_cells;
  p.spec_cs = b->spec_cs;
  p.spec_meta = b->spec_meta;
  p.ds = b->ds;
  p.peer = b->peer;
  return p;
}
// ... and for a fanout_kernel launch
FanParams fan_params(const rb_p2p* b) {
  FanParams fp{};
  fp.status = b->status;
  fp.snap = b->snap;
  fp.tag = b->tag;
  fp.ring = b->ring;
  fp.qs = b->qs;
  fp.spec_state = b->spec_state;
  fp.spec_cells = b->spec_cells;
  fp.spec_cs = b->spec_cs;
  fp.spec_meta = b->spec_meta;
  fp.stats = b->stats;
  fp.counters = b->counters;
  fp.S = b->S;
  fp.Spad = b->Spad;
  fp.W = b->W;
  fp.local_mask = b->cfg.local_mask;
  fp.fan_generic = b->fan_generic ? 1 : 0;
  fp.fan_k = b->cfg.fanout_candidates;
  return fp;
}
}  // namespace

namespace {
// The adaptive fan-out (include/ggrs_amd.h RB_P2P_FLAG_FANOUT_ALWAYS).  Windows of kFanProbeTicks
// ticks back to back while presimulating; each window's select and LoadGameState sums are reduced on
// the device into pinned memory at its end (host[2..3], event `ev`) and its start (host[0..1]: the
// previous window's end).  The decision is taken kFanDecideTicks ticks after a window's end, at the
// first call from then on, waiting for the event (long complete by then): so whether a tick
// speculates depends only on the batch's inputs and call sizes, never on when a copy landed.
constexpr int32_t kFanDecideTicks = 16;
rb_status fan_snapshot(rb_p2p* b, int off) {
  RB_TRY(b, hipMemsetAsync(b->fan.dev + off, 0, 2 * sizeof(unsigned long long), b->stream));
  hipLaunchKernelGGL(fan_sums_kernel, dim3((b->S + 255) / 256), dim3(256), 0, b->stream, b->stats, b->S, b->Spad,
                     b->fan.dev + off);
  RB_TRY(b, hipGetLastError());
  RB_TRY(b, hipMemcpyAsync(b->fan.host + off, b->fan.dev + off, 2 * sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, b->stream));
  return RB_OK;
}
// Branches are valid only for the tick right after the launch that made them (SM_END == current
// frame); a pause's plain ticks leave the metadata as it was, so it is cleared when presimulation
// stops and again when it restarts.
rb_status fan_invalidate(rb_p2p* b) {
  RB_TRY(b, hipMemsetAsync(b->spec_meta + static_cast<size_t>(SM_VALID) * b->Spad, 0, static_cast<size_t>(b->Spad) * 4,
                           b->stream));
  return RB_OK;
}
rb_status fan_before(rb_p2p* b) {
  auto& f = b->fan;
  if (!f.adaptive) return RB_OK;
  if (f.pending && f.since_end >= kFanDecideTicks) {
    RB_TRY(b, hipEventSynchronize(f.ev));
    f.pending = false;
    const uint64_t sel = f.host[2] - f.host[0], ld = f.host[3] - f.host[1];
    f.windows += 1;
    if (sel + ld >= kFanMinRollbacks) {
      f.last_frac = static_cast<double>(sel) / static_cast<double>(sel + ld);
      if (sel * 1000ull < static_cast<uint64_t>(f.min_permille) * (sel + ld)) {
        f.active = false;  // a pause of kFanPauseTicks plain ticks
        f.open = false;
        f.ticks = 0;
        f.turned_off += 1;
        rb_status r = fan_invalidate(b);
        if (r != RB_OK) return r;
      }
    }
    if (f.active) {  // the next window started at this one's end
      f.host[0] = f.host[2];
      f.host[1] = f.host[3];
    }
  }
  if (!f.active && f.ticks >= kFanPauseTicks) {  // measure again
    f.active = true;
    f.open = false;
    rb_status r = fan_invalidate(b);
    if (r != RB_OK) return r;
  }
  if (f.active && !f.open) {
    rb_status r = fan_snapshot(b, 0);
    if (r != RB_OK) return r;
    f.open = true;
    f.ticks = 0;
  }
  return RB_OK;
}
rb_status fan_after(rb_p2p* b, int32_t n) {
  auto& f = b->fan;
  if (!f.adaptive) return RB_OK;
  f.ticks += n;
  if (f.pending) f.since_end += n;
  if (f.active && f.open && !f.pending && f.ticks >= kFanProbeTicks) {
    rb_status r = fan_snapshot(b, 2);
    if (r != RB_OK) return r;
    RB_TRY(b, hipEventRecord(f.ev, b->stream));
    f.pending = true;
    f.since_end = 0;
    f.ticks = 0;
  }
  return RB_OK;
}
}  // namespace

namespace {
constexpr const char* kTsOff = "time sync is off (rb_p2p_time_sync_enable)";
constexpr const char* kLvOff = "liveness is off (rb_p2p_liveness_enable)";
constexpr const char* kRingFrames =
    "the batch has a delivery ring (rb_p2p_set_delivery_ring): the by-frame tensor holds exactly ring_frames frames";
// The tick log for a call of n ticks.  It grows to the largest call seen, and only once the stream
// is idle: the launches before this call may still read the old one.
rb_status ts_log_reserve(rb_p2p* b, int32_t n) {
  if (n <= b->ts_log_ticks) return RB_OK;
  RB_TRY(b, hipStreamSynchronize(b->stream));
  b->ts_log_ticks = 0;
  RB_TRY(b, b->res.release(b->ts_log));
  const size_t bytes = static_cast<size_t>(n) * kTlRows * b->Spad * 4;
  RB_TRY(b, b->res.alloc(b->ts_log, bytes));
  RB_TRY(b, hipMemsetAsync(b->ts_log, 0xff, bytes, b->stream));  // kTlUnwritten
  b->ts_log_ticks = n;
  return RB_OK;
}
// p2p_time_sync_kernel over the n ticks the P2P launch(es) of this call just logged
rb_status ts_launch(rb_p2p* b, const P2PParams& p, int32_t n, const int32_t* status = nullptr) {
  const dim3 grid((b->Spad + 255) / 256), block(256);  // lanes past S do nothing
  auto k = b->P == 1 ? p2p_time_sync_kernel<1> : b->P == 2 ? p2p_time_sync_kernel<2>
         : b->P == 3 ? p2p_time_sync_kernel<3> : p2p_time_sync_kernel<4>;
  hipLaunchKernelGGL(k, grid, block, 0, b->stream, b->ts, b->ts_log, static_cast<int64_t>(kTlRows) * b->Spad, p.upto, p.upto_stride, status ? status : b->status, n,
                     b->S, b->Spad, p.remote_frames, b->cfg.local_mask, b->cfg.input_delay, b->peer.on);
  RB_TRY(b, hipGetLastError());
  return RB_OK;
}

// What every rb_p2p_run_ticks* call starts with, inside its DeviceScope: the batch's parameters with
// the caller's tensors, the tick log for `log_ticks` ticks of the call when time sync is on, and the
// profiling event pair (null when the batch is not profiling; consumed only by prof_ev.commit()).
rb_status tick_params(rb_p2p* b, int32_t T, const void* local_inputs, int64_t local_stride, const int32_t* remote_upto,
                      const void* remote_inputs, int32_t remote_frames, int32_t log_ticks, P2PParams& p, LaunchEv& ev) {
  p = base_params(b);
  p.local_in = static_cast<const uint8_t*>(local_inputs);
  p.local_stride = local_stride;
  p.upto = remote_upto;
  p.upto_stride = static_cast<int64_t>(b->P) * b->S;
  p.remote_in = static_cast<const uint8_t*>(remote_inputs);
  // a delivery ring: no frame is clamped to the tensor's length, frame f sits in slot f & (R - 1)
  p.remote_frames = b->ring_frames ? INT32_MAX : remote_frames;
  p.remote_mask = b->ring_frames ? b->ring_frames - 1 : INT32_MAX;
  p.T = T;
  if (b->ts_on) {
    rb_status r = ts_log_reserve(b, log_ticks);
    if (r != RB_OK) return r;
    p.tick_log = b->ts_log;
  }
  b->ticked = true;
  if (b->prof) RB_TRY(b, b->prof_ev.next(ev));
  return RB_OK;
}
}  // namespace

rb_status rb_p2p_fanout_state(rb_p2p* b, int32_t* active, double* select_fraction, int32_t* windows,
                              int32_t* turned_off) {
  if (!b->fanout) return fail(b, RB_INVALID_REQUEST, "the batch has no fan-out");
  if (active) *active = (!b->fan.adaptive || b->fan.active) ? 1 : 0;
  if (select_fraction) *select_fraction = b->fan.last_frac;
  if (windows) *windows = b->fan.windows;
  if (turned_off) *turned_off = b->fan.turned_off;
  return RB_OK;
}

rb_status rb_p2p_run_ticks(rb_p2p* b, int32_t n_ticks, const void* local_inputs, int64_t local_stride,
                           const int32_t* remote_upto, const void* remote_inputs, int32_t remote_frames) {
  if (n_ticks <= 0) return RB_OK;
  if (!local_inputs || !remote_upto || !remote_inputs || remote_frames <= 0)
    return fail(b, RB_INVALID_REQUEST, "rb_p2p_run_ticks: missing input tensor");
  if (b->ring_frames && remote_frames != b->ring_frames) return fail(b, RB_INVALID_REQUEST, kRingFrames);
  DeviceScope dev_scope(b->device);
  P2PParams p;
  LaunchEv ev;
  rb_status r = tick_params(b, n_ticks, local_inputs, local_stride, remote_upto, remote_inputs, remote_frames, n_ticks, p, ev);
  if (r == RB_OK && b->fanout) r = fan_before(b);
  if (r != RB_OK) return r;
  const bool spec = b->fanout && (!b->fan.adaptive || b->fan.active);
  p.spec_on = spec ? 1 : 0;
  const bool one_launch = !spec || (b->ops->inlane_fanout && !b->fan_generic);
  hipError_t e = hipSuccess;
  if (one_launch) {
    // all ticks in one launch (with the in-kernel fan-out); timed by the kernel's own start / end
    p.launch_clock = b->clock.next();
    e = b->ops->launch_p2p(p, b->block, b->stream, ev);
  } else {
    if (ev.start) RB_TRY(b, hipEventRecord(ev.start, b->stream));
    // fanout_kernel between ticks needs every lane of a session's branches: one
    // P2P launch and one fan-out launch per tick
    FanParams fp = fan_params(b);
    P2PParams pt = p;
    pt.T = 1;
    for (int32_t t = 0; t < n_ticks && e == hipSuccess; ++t) {
      pt.local_in = p.local_in + static_cast<int64_t>(t) * p.local_stride;
      pt.upto = p.upto + static_cast<int64_t>(t) * p.upto_stride;
      if (p.tick_log) pt.tick_log = p.tick_log + static_cast<int64_t>(t) * kTlRows * b->Spad;  // this tick's rows
      pt.launch_clock = b->clock.next();
      e = b->ops->launch_p2p(pt, b->block, b->stream);
      fp.launch_clock = b->clock.next();
      if (e == hipSuccess) e = b->ops->launch_fanout(fp, b->block, b->stream);
    }
  }
  if (e != hipSuccess) return fail(b, RB_DEVICE_ERROR, std::string("p2p launch: ") + hipGetErrorString(e));
  if (ev.stop && !one_launch) RB_TRY(b, hipEventRecord(ev.stop, b->stream));
  if (ev.start) b->prof_ev.commit();  // only a launch that went out has its event pair recorded
  if (b->ts_on) {
    r = ts_launch(b, p, n_ticks);
    if (r != RB_OK) return r;
  }
  if (b->fanout) return fan_after(b, n_ticks);
  return RB_OK;
}

rb_status rb_p2p_run_ticks_paced(rb_p2p* b, int32_t n_ticks, const void* local_inputs, int64_t local_stride,
                                 const int32_t* remote_upto, const void* remote_inputs, int32_t remote_frames,
                                 const uint8_t* run_mask) {
  if (!run_mask) return rb_p2p_run_ticks(b, n_ticks, local_inputs, local_stride, remote_upto, remote_inputs, remote_frames);
  if (n_ticks <= 0) return RB_OK;
  if (!local_inputs || !remote_upto || !remote_inputs || remote_frames <= 0)
    return fail(b, RB_INVALID_REQUEST, "rb_p2p_run_ticks_paced: missing input tensor");
  if (b->ring_frames && remote_frames != b->ring_frames) return fail(b, RB_INVALID_REQUEST, kRingFrames);
  if (b->fanout)  // the move-to-front rows and branch validity under a parked poll: a later step
    return fail(b, RB_INVALID_REQUEST, "rb_p2p_run_ticks_paced: a batch with the fan-out takes rb_p2p_run_ticks");
  const int IB = b->ops->input_bytes;
  if (IB != 1 && IB != 4) return fail(b, RB_INVALID_REQUEST, "rb_p2p_run_ticks_paced: inputs of 1 or 4 bytes");
  DeviceScope dev_scope(b->device);
  rb_status r = pace_reserve(b);
  if (r != RB_OK) return r;
  P2PParams p;
  LaunchEv ev;
  // (one row of the tick log, consumed by every tick's own time-sync launch)
  r = tick_params(b, 1, local_inputs, local_stride, remote_upto, remote_inputs, remote_frames, 1, p, ev);
  if (r != RB_OK) return r;
  p.status = b->pace.view;  // parked sessions read as panicked: p2p_kernel returns before any store
  if (ev.start) RB_TRY(b, hipEventRecord(ev.start, b->stream));
  const dim3 grid((b->S + 255) / 256), block(256);
  auto poll = IB == 1 ? poll_kernel_of<1>(b->P) : poll_kernel_of<4>(b->P);
  const TimeSyncParams ts = b->ts_on ? b->ts : TimeSyncParams{};
  // n_ticks one-tick sequences on the stream.  p2p_time_sync_kernel keeps a session's advantages in
  // registers from entry to exit and ends its walk at the first unwritten row (a parked tick's), so
  // it runs once per tick, on that tick's row; and it reads the view, not the status array, which
  // does not have this tick's panics of the running sessions until p2p_unpark_kernel has run.
  for (int32_t t = 0; t < n_ticks; ++t) {
    const uint8_t* const mask = run_mask + static_cast<int64_t>(t) * b->S;
    p.local_in = static_cast<const uint8_t*>(local_inputs) + static_cast<int64_t>(t) * local_stride;
    p.upto = remote_upto + static_cast<int64_t>(t) * p.upto_stride;
    hipLaunchKernelGGL(poll, grid, block, 0, b->stream, b->pace, mask, b->qs, static_cast<uint8_t*>(b->ring), b->status,
                       b->counters, p.upto, p.remote_in, p.remote_frames, p.remote_mask, b->cfg.remote_delay,
                       b->cfg.local_mask, ts, b->S, b->Spad);
    RB_TRY(b, hipGetLastError());
    p.launch_clock = b->clock.next();
    const hipError_t e = b->ops->launch_p2p(p, b->block, b->stream);
    if (e != hipSuccess) return fail(b, RB_DEVICE_ERROR, std::string("p2p launch: ") + hipGetErrorString(e));
    if (b->ts_on) {
      r = ts_launch(b, p, 1, b->pace.view);
      if (r != RB_OK) return r;
    }
    hipLaunchKernelGGL(p2p_unpark_kernel, grid, block, 0, b->stream, b->pace.view, mask, b->status, b->S);
    RB_TRY(b, hipGetLastError());
  }
  if (ev.stop) {
    RB_TRY(b, hipEventRecord(ev.stop, b->stream));
    b->prof_ev.commit();
  }
  return RB_OK;
}

rb_status rb_p2p_pace(rb_p2p* b, uint8_t* run_mask_dev) {
  if (!b->ts_on) return fail(b, RB_INVALID_REQUEST, kTsOff);
  if (!run_mask_dev) return fail(b, RB_INVALID_REQUEST, "rb_p2p_pace: missing run mask");
  DeviceScope dev_scope(b->device);
  rb_status r = pace_reserve(b);
  if (r != RB_OK) return r;
  hipLaunchKernelGGL(p2p_pace_kernel, dim3((b->S + 255) / 256), dim3(256), 0, b->stream, b->pace, b->ts.state, b->status,
                     run_mask_dev, b->S, b->Spad);
  RB_TRY(b, hipGetLastError());
  return RB_OK;
}

rb_status rb_p2p_read_pacing(rb_p2p* b, uint32_t* parked_ticks) {
  if (!parked_ticks) return RB_OK;
  DeviceScope dev_scope(b->device);
  if (!b->pace.parked) {  // no paced tick yet
    RB_TRY(b, hipStreamSynchronize(b->stream));
    std::memset(parked_ticks, 0, static_cast<size_t>(b->S) * 4);
    return RB_OK;
  }
  std::vector<uint32_t> v;
  rb_status r = read_rows(b, b->pace.parked, 1, v);
  if (r != RB_OK) return r;
  std::memcpy(parked_ticks, v.data(), static_cast<size_t>(b->S) * 4);
  return RB_OK;
}

rb_status rb_p2p_run_ticks_packets(rb_p2p* b, int32_t n_ticks, const void* local_inputs, int64_t local_stride,
                                   const uint8_t* packets, int64_t packet_stride, const int32_t* lengths,
                                   const int32_t* start_frames, int32_t* decode_status, int32_t* acks) {
  if (n_ticks <= 0) return RB_OK;
  if (!local_inputs || !packets || !lengths || !start_frames)
    return fail(b, RB_INVALID_REQUEST, "rb_p2p_run_ticks_packets: missing input tensor");
  if (packet_stride < 32 || packet_stride % 16 != 0 || reinterpret_cast<uintptr_t>(packets) % 16 != 0)
    return fail(b, RB_INVALID_REQUEST, "rb_p2p_run_ticks_packets: packets need 16-byte alignment and a stride of at least 32");
  if (b->cfg.sparse_saving || b->fanout || b->ds.interval > 0 || b->peer.on)
    return fail(b, RB_INVALID_REQUEST,
                "rb_p2p_run_ticks_packets: sparse saving, the fan-out and network reports take rb_p2p_run_ticks");
  if (b->ts_on)  // last_recv_frame is decided inside the kernel there
    return fail(b, RB_INVALID_REQUEST, "rb_p2p_run_ticks_packets: time sync takes rb_p2p_run_ticks");
  // a packet's reference input (frame start - 1) may be as old as the newest received frame -
  // 2 * max_prediction (recv_inputs' retain, protocol.rs:684-686); the 128-entry input queue ring
  // holds the newest 128 frames, so that frame must be younger than last - 127
  if (2 * b->W >= kQueueLen)
    return fail(b, RB_INVALID_REQUEST, "rb_p2p_run_ticks_packets: needs 2 * max_prediction < 128 (the input ring)");
  DeviceScope dev_scope(b->device);
  P2PParams p;
  LaunchEv ev;  // the kernel's own start / end (hipExtLaunchKernel)
  rb_status r = tick_params(b, n_ticks, local_inputs, local_stride, nullptr, nullptr, 0, n_ticks, p, ev);
  if (r != RB_OK) return r;
  p.packets = packets;
  p.packet_stride = packet_stride;
  p.pk_len = lengths;
  p.pk_start = start_frames;
  p.pk_status = decode_status;
  p.acks = acks;
  p.launch_clock = b->clock.next();
  hipError_t e = b->ops->launch_p2p(p, b->block, b->stream, ev);
  if (e != hipSuccess) return fail(b, RB_DEVICE_ERROR, std::string("p2p launch: ") + hipGetErrorString(e));
  if (ev.start) b->prof_ev.commit();  // only a launch that went out has its event pair recorded
  return RB_OK;
}

rb_status rb_p2p_disconnect_player(rb_p2p* b, int32_t handle, const uint8_t* session_mask) {
  if (handle < 0 || handle >= b->P) return fail(b, RB_INVALID_REQUEST, "Invalid Player Handle.");
  if ((b->cfg.local_mask >> handle) & 1u) return fail(b, RB_INVALID_REQUEST, "Local Player cannot be disconnected.");
  DeviceScope dev_scope(b->device);
  if (b->peer.on || b->mirror_stale) {  // peers' reports disconnect players inside the ticks, an import brings its own: refresh the mirror
    std::vector<int32_t> qs;
    rb_status r = read_rows(b, b->qs, kQsFields, qs);
    if (r != RB_OK) return r;
    for (int h = 0; h < b->P; ++h)
      for (int s = 0; s < b->S; ++s)
        b->disconnected[static_cast<size_t>(h) * b->S + s] = (static_cast<uint32_t>(qs[(QS_PLAYER0 + QF_MISC * 4 + h) * b->Spad + s]) & kQmDisc) != 0;
    b->mirror_stale = false;
  }
  uint8_t* d = b->disconnected.data() + static_cast<size_t>(handle) * b->S;
  for (int s = 0; s < b->S; ++s)
    if ((!session_mask || session_mask[s]) && d[s]) return fail(b, RB_INVALID_REQUEST, "Player already disconnected.");
  for (int s = 0; s < b->S; ++s)
    if (!session_mask || session_mask[s]) d[s] = 1;
  if (session_mask) {
    RB_TRY(b, hipMemcpyAsync(b->disc_mask, session_mask, b->S, hipMemcpyHostToDevice, b->stream));
    RB_TRY(b, hipStreamSynchronize(b->stream));  // the host mask may be reused as soon as we return
  }
  const int blocks = (b->S + 255) / 256;
  hipLaunchKernelGGL(p2p_disconnect_kernel, dim3(blocks), dim3(256), 0, b->stream, b->qs,
                     session_mask ? b->disc_mask : nullptr, b->S, b->Spad, handle);
  RB_TRY(b, hipGetLastError());
  return RB_OK;
}

rb_status rb_p2p_restart_sessions(rb_p2p* b, const uint8_t* session_mask) {
  std::vector<int32_t> idx;
  const rb_status r = restart_sessions(b, session_mask, idx);
  if (r != RB_OK) return r;
  // the host mirror of ConnectionStatus::disconnected
  if (!session_mask) std::fill(b->disconnected.begin(), b->disconnected.end(), uint8_t{0});
  for (int h = 0; h < b->P; ++h)
    for (int32_t s : idx) b->disconnected[static_cast<size_t>(h) * b->S + s] = 0;
  return RB_OK;
}

// ---- moving sessions between batches (migrate.hpp).  GGRS has no such call: a P2PSession is an
// ordinary movable Rust value.

// The configuration the kernels compile in or read: a record goes only into a batch that agrees.
std::vector<uint32_t> rb_p2p::record_config() const {
  const rb_p2p* const b = this;
  const GameOps& o = *b->ops;
  std::vector<uint32_t> cfg{1u /* a P2P batch */,
          static_cast<uint32_t>(b->cfg.game),
          static_cast<uint32_t>(b->P),
          static_cast<uint32_t>(b->W),
          static_cast<uint32_t>(o.input_bytes),
          static_cast<uint32_t>(o.nw),
          static_cast<uint32_t>(o.lanes),
          static_cast<uint32_t>(o.cs_bytes),
          static_cast<uint32_t>(o.image_bytes),
          static_cast<uint32_t>(b->cfg.input_delay),
          static_cast<uint32_t>(b->cfg.remote_delay),
          b->cfg.local_mask,
          b->cfg.sparse_saving ? 1u : 0u,
          static_cast<uint32_t>(b->ds.interval),
          b->peer.on ? 1u : 0u,
          b->ts_on ? 1u : 0u,
          b->ts_on ? static_cast<uint32_t>(b->ts.fps) : 0u,
          b->fanout ? (b->per_player ? 2u : 1u) : 0u,
          b->fanout ? static_cast<uint32_t>(b->cfg.fanout_candidates) : 0u};
  // (appended only with liveness on: a batch without it keeps the record and fingerprint it had)
  if (b->lv_on) {
    cfg.push_back(1u);
    cfg.push_back(static_cast<uint32_t>(b->lv.timeout_ms));
    cfg.push_back(static_cast<uint32_t>(b->lv.notify_ms));
  }
  return cfg;
}

// the groups a later call would make, with create's fresh values: record_bytes depends on the
// configuration only, and no read-back of a batch that never paces or exports changes
rb_status rb_p2p::before_move() {
  const rb_status r = export_reserve(this);
  return r == RB_OK && !fanout ? pace_reserve(this) : r;
}

int64_t rb_p2p_session_record_bytes(const rb_p2p* b) {
  PlaneSet ps;  // (layout only: nothing of the batch is written)
  return static_cast<int64_t>(record_planes(const_cast<rb_p2p*>(b), ps, true).record_bytes);
}

rb_status rb_p2p_export_sessions(rb_p2p* b, const int32_t* sessions, int32_t n, void* records_dev) {
  return move_sessions(b, sessions, n, records_dev, false);
}

rb_status rb_p2p_import_sessions(rb_p2p* b, const int32_t* sessions, int32_t n, const void* records_dev) {
  const rb_status r = move_sessions(b, sessions, n, const_cast<void*>(records_dev), true);
  if (r == RB_OK && n > 0) {
    b->ticked = true;        // the columns hold a running match: rb_p2p_time_sync_enable is closed
    b->mirror_stale = true;  // ConnectionStatus::disconnected arrived in qs
  }
  return r;
}

rb_status rb_p2p_import_refused(rb_p2p* b, uint32_t* count) { return import_refused(b, count); }

rb_status rb_p2p_read_status(rb_p2p* b, int32_t* status, int32_t* load_frame, int32_t* n_adv, int32_t* n_save) {
  std::vector<int32_t> st, tr, cur;
  rb_status r = read_rows(b, b->status, 1, st);
  if (r == RB_OK) r = read_rows(b, b->trace, 1, tr);
  if (r == RB_OK) r = read_rows(b, b->qs + QS_CUR * b->Spad, 1, cur);
  if (r != RB_OK) return r;
  for (int s = 0; s < b->S; ++s) {  // trace_pack
    const uint32_t t = static_cast<uint32_t>(tr[s]);
    const int32_t na = static_cast<int32_t>((t >> 16) & 0xFFu), ns = static_cast<int32_t>(t >> 24);
    if (status) status[s] = st[s] == kP2PStatusPanic ? RB_PANIC : st[s];
    if (load_frame) load_frame[s] = fd_dec(t, cur[s]);
    if (n_adv) n_adv[s] = na == 0xFF ? -1 : na;
    if (n_save) n_save[s] = ns == 0xFF ? -1 : ns;
  }
  return RB_OK;
}

rb_status rb_p2p_read_frames(rb_p2p* b, int32_t* current, int32_t* confirmed) {
  std::vector<int32_t> qs;
  rb_status r = read_rows(b, b->qs, kQsFields, qs);
  if (r != RB_OK) return r;
  for (int s = 0; s < b->S; ++s) {
    if (current) current[s] = qs[QS_CUR * b->Spad + s];
    if (confirmed) {
      const size_t Sp = b->Spad;
      const uint32_t sc = static_cast<uint32_t>(qs[QS_SAVED_CONF * Sp + s]);
      confirmed[s] = sc == kQsEscWord ? qs[QS_ABS_CONF * Sp + s] : fd_dec(sc >> 16, qs[QS_CUR * Sp + s]);
    }
  }
  return RB_OK;
}

rb_status rb_p2p_read_queues(rb_p2p* b, int32_t* out) {
  std::vector<int32_t> qs;
  rb_status r = read_rows(b, b->qs, kQsFields, qs);
  if (r != RB_OK) return r;
  static_assert(RB_P2P_QUEUE_FIELDS == 8, "last added, tail, length, last requested, prediction, first incorrect, connection, disconnected");
  const size_t Sp = b->Spad;
  for (int s = 0; s < b->S; ++s)
    for (int h = 0; h < b->P; ++h) {
      auto row = [&](int field) { return qs[(QS_PLAYER0 + field * 4 + h) * Sp + s]; };
      uint32_t w[4];
      int32_t ab[7];
      for (int i = 0; i < 4; ++i) w[i] = static_cast<uint32_t>(row(QF_LA_CONN + i));
      for (int i = 0; i < 7; ++i) ab[i] = row(QF_ABS0 + i);
      const QFields f = q_unpack(w, qs[QS_CUR * Sp + s], ab);
      const int32_t v[RB_P2P_QUEUE_FIELDS] = {f.la, f.tail, f.len, f.req, f.pred, f.fi, f.conn, f.disc ? 1 : 0};
      for (int k = 0; k < RB_P2P_QUEUE_FIELDS; ++k) out[(static_cast<size_t>(s) * b->P + h) * RB_P2P_QUEUE_FIELDS + k] = v[k];
    }
  return RB_OK;
}

rb_status rb_p2p_read_cells(rb_p2p* b, int32_t* tags, void* images, uint64_t* checksums) {
  DeviceScope dev_scope(b->device);
  std::vector<int32_t> tg;
  rb_status r = read_rows(b, b->tag, b->W, tg);
  if (r != RB_OK) return r;
  const size_t Sp = b->Spad, L = b->ops->lanes, NW = b->ops->nw, B = b->ops->image_bytes;
  std::vector<uint8_t> csh(b->W * Sp * b->ops->cs_bytes);
  RB_TRY(b, hipMemcpy(csh.data(), b->cs, csh.size(), hipMemcpyDeviceToHost));
  std::vector<uint32_t> planes;
  for (int w = 0; w < b->W; ++w) {
    if (images) {
      r = read_rows(b, b->snap + static_cast<size_t>(w) * NW * Sp * L, NW * L, planes);
      if (r != RB_OK) return r;
    }
    for (int s = 0; s < b->S; ++s) {
      const int32_t f = tg[w * Sp + s];
      if (tags) tags[static_cast<size_t>(w) * b->S + s] = f;
      if (images) image_from_planes(b, planes, s, f, static_cast<uint8_t*>(images) + (static_cast<size_t>(w) * b->S + s) * B);
      if (checksums) {
        const U128 c = b->ops->cs_at(csh.data(), static_cast<size_t>(w) * Sp + s);
        checksums[(static_cast<size_t>(w) * b->S + s) * 2] = c.lo;
        checksums[(static_cast<size_t>(w) * b->S + s) * 2 + 1] = c.hi;
      }
    }
  }
  return RB_OK;
}

rb_status rb_p2p_read_live(rb_p2p* b, void* images) {
  std::vector<int32_t> qs;
  std::vector<uint32_t> planes;
  rb_status r = read_rows(b, b->qs, kQsFields, qs);
  if (r == RB_OK) r = read_rows(b, b->live, static_cast<size_t>(b->ops->nw) * b->ops->lanes, planes);
  if (r != RB_OK) return r;
  for (int s = 0; s < b->S; ++s)
    image_from_planes(b, planes, s, qs[QS_CUR * b->Spad + s],
                      static_cast<uint8_t*>(images) + static_cast<size_t>(s) * b->ops->image_bytes);
  return RB_OK;
}

rb_status rb_p2p_counters(rb_p2p* b, uint32_t* out3) {
  uint32_t c[4];
  DeviceScope dev_scope(b->device);
  RB_TRY(b, hipStreamSynchronize(b->stream));
  RB_TRY(b, hipMemcpy(c, b->counters, 16, hipMemcpyDeviceToHost));
  for (int i = 0; i < 3; ++i) out3[i] = c[i];
  return RB_OK;
}

rb_status rb_p2p_totals(rb_p2p* b, uint64_t* out5) {
  std::vector<unsigned long long> st;
  rb_status r = read_rows(b, b->stats, ST_COUNT, st);
  if (r != RB_OK) return r;
  for (int i = 0; i < ST_COUNT; ++i) {
    uint64_t t = 0;
    for (int s = 0; s < b->S; ++s) t += st[static_cast<size_t>(i) * b->Spad + s];
    out5[i] = t;
  }
  return RB_OK;
}

rb_status rb_p2p_take_checksum_reports(rb_p2p* b, void* dev_out) {
  if (b->ds.interval <= 0) return fail(b, RB_INVALID_REQUEST, "desync detection is off (desync_interval = 0)");
  DeviceScope dev_scope(b->device);
  hipLaunchKernelGGL(p2p_take_reports_kernel, dim3((b->S + 255) / 256), dim3(256), 0, b->stream, b->ds,
                     static_cast<rb_checksum_report*>(dev_out), b->S, b->Spad);
  RB_TRY(b, hipGetLastError());
  return RB_OK;
}

rb_status rb_p2p_receive_checksum_reports(rb_p2p* b, int32_t handle, const void* dev_in, int32_t count) {
  if (b->ds.interval <= 0) return fail(b, RB_INVALID_REQUEST, "desync detection is off (desync_interval = 0)");
  if (handle < 0 || handle >= b->P || ((b->cfg.local_mask >> handle) & 1u))
    return fail(b, RB_INVALID_REQUEST, "checksum reports come from a remote handle's endpoint");
  if (count <= 0) return RB_OK;
  DeviceScope dev_scope(b->device);
  hipLaunchKernelGGL(p2p_receive_reports_kernel, dim3((b->S + 255) / 256), dim3(256), 0, b->stream, b->ds,
                     static_cast<const rb_checksum_report*>(dev_in), count, b->S, b->Spad, handle);
  RB_TRY(b, hipGetLastError());
  return RB_OK;
}

rb_status rb_p2p_receive_peer_connect_status(rb_p2p* b, int32_t endpoint, const int32_t* last_frames,
                                             const uint8_t* disconnected) {
  if (!b->peer.on) return fail(b, RB_INVALID_REQUEST, "peer connect status needs RB_P2P_FLAG_PEER_STATUS");
  if (endpoint < 0 || endpoint >= b->P || ((b->cfg.local_mask >> endpoint) & 1u))
    return fail(b, RB_INVALID_REQUEST, "connect-status reports come from a remote handle's endpoint");
  if (!last_frames || !disconnected) return fail(b, RB_INVALID_REQUEST, "missing connect-status tensor");
  DeviceScope dev_scope(b->device);
  hipLaunchKernelGGL(p2p_peer_status_kernel, dim3((b->S + 255) / 256), dim3(256), 0, b->stream, b->peer, last_frames,
                     disconnected, b->S, b->Spad, b->P, endpoint);
  RB_TRY(b, hipGetLastError());
  return RB_OK;
}

rb_status rb_p2p_export_confirmed_inputs(rb_p2p* b, void* inputs_by_frame, int32_t frames, int32_t* upto,
                                         int32_t* last_frames, uint8_t* disconnected) {
  if (!inputs_by_frame || !upto || !last_frames || !disconnected || frames <= 0)
    return fail(b, RB_INVALID_REQUEST, "rb_p2p_export_confirmed_inputs: missing output tensor");
  if (b->ring_frames && frames != b->ring_frames) return fail(b, RB_INVALID_REQUEST, kRingFrames);
  DeviceScope dev_scope(b->device);
  if (rb_status r = export_reserve(b); r != RB_OK) return r;
  const dim3 grid((b->S + 255) / 256), block(256);
  auto k = b->ops->input_bytes == 4 ? p2p_export_kernel<4> : p2p_export_kernel<1>;
  if (b->ops->input_bytes != 4 && b->ops->input_bytes != 1)
    return fail(b, RB_INVALID_REQUEST, "rb_p2p_export_confirmed_inputs: 1- and 4-byte inputs");
  hipLaunchKernelGGL(k, grid, block, 0, b->stream, b->qs, static_cast<const uint8_t*>(b->ring), b->status, b->exp_state,
                     b->S, b->Spad, b->P, static_cast<uint8_t*>(inputs_by_frame), frames, b->ring_frames, upto, last_frames,
                     disconnected);
  RB_TRY(b, hipGetLastError());
  return RB_OK;
}

rb_status rb_p2p_set_delivery_ring(rb_p2p* b, int32_t ring_frames) {
  if (ring_frames != 0 && (ring_frames < RB_INPUT_QUEUE_LENGTH || (ring_frames & (ring_frames - 1)) != 0))
    return fail(b, RB_INVALID_REQUEST, "rb_p2p_set_delivery_ring: ring_frames is 0 or a power of two of at least 128");
  if (ring_frames != 0 && b->cfg.game >= RB_GAME_PLUGIN_BASE && !plugin_masks_delivery_frames(b->cfg.game))
    return fail(b, RB_INVALID_REQUEST, "rb_p2p_set_delivery_ring: rebuild the game plugin against the current headers");
  b->ring_frames = ring_frames;
  return RB_OK;
}

rb_status rb_p2p_export_local_inputs(rb_p2p* b, void* inputs_by_frame, int32_t frames, int32_t* sent) {
  if (!inputs_by_frame || !sent || frames <= 0)
    return fail(b, RB_INVALID_REQUEST, "rb_p2p_export_local_inputs: missing tensor");
  if (b->ring_frames && frames != b->ring_frames) return fail(b, RB_INVALID_REQUEST, kRingFrames);
  if (b->ops->input_bytes != 4 && b->ops->input_bytes != 1)
    return fail(b, RB_INVALID_REQUEST, "rb_p2p_export_local_inputs: 1- and 4-byte inputs");
  DeviceScope dev_scope(b->device);
  const dim3 grid((b->S + 255) / 256), block(256);
  auto k = b->ops->input_bytes == 4 ? p2p_export_local_kernel<4> : p2p_export_local_kernel<1>;
  hipLaunchKernelGGL(k, grid, block, 0, b->stream, b->qs, static_cast<const uint8_t*>(b->ring), b->status, b->S, b->Spad,
                     b->P, b->cfg.local_mask, static_cast<uint8_t*>(inputs_by_frame), frames, b->ring_frames, sent);
  RB_TRY(b, hipGetLastError());
  return RB_OK;
}

rb_status rb_p2p_read_export_status(rb_p2p* b, int32_t* status, int32_t* next_frame) {
  if (!b->exp_state) {  // no export yet
    for (int s = 0; s < b->S; ++s) {
      if (status) status[s] = RB_P2P_EXPORT_OK;
      if (next_frame) next_frame[s] = 0;
    }
    return RB_OK;
  }
  std::vector<int32_t> st;
  rb_status r = read_rows(b, b->exp_state, 2, st);
  if (r != RB_OK) return r;
  for (int s = 0; s < b->S; ++s) {
    if (next_frame) next_frame[s] = st[s];
    if (status) status[s] = st[static_cast<size_t>(b->Spad) + s];
  }
  return RB_OK;
}

// ---- time sync (time_sync.hpp)
rb_status rb_p2p_time_sync_enable(rb_p2p* b, int32_t fps) {
  if (fps <= 0) return fail(b, RB_INVALID_REQUEST, "FPS should be higher than 0.");  // builder.rs:190-194
  if (b->ts_on) return fail(b, RB_INVALID_REQUEST, "rb_p2p_time_sync_enable: time sync is already on");
  if (b->ticked) return fail(b, RB_INVALID_REQUEST, "rb_p2p_time_sync_enable: comes before the batch's first tick");
  if (b->cfg.game >= RB_GAME_PLUGIN_BASE && !plugin_writes_tick_log(b->cfg.game))
    return fail(b, RB_INVALID_REQUEST, "rb_p2p_time_sync_enable: rebuild the game plugin against the current headers");
  DeviceScope dev_scope(b->device);
  b->ts.fps = fps;
  if (const rb_status r = make_group(b, time_sync_planes); r != RB_OK) return r;
  b->ts_on = true;
  return RB_OK;
}

rb_status rb_p2p_receive_quality(rb_p2p* b, int32_t handle, const int32_t* rtt_ms, const int32_t* frame_advantage) {
  if (!b->ts_on) return fail(b, RB_INVALID_REQUEST, kTsOff);
  if (handle < 0 || handle >= b->P || ((b->cfg.local_mask >> handle) & 1u))
    return fail(b, RB_INVALID_REQUEST, "quality reports come from a remote handle's endpoint");
  if (!rtt_ms && !frame_advantage) return RB_OK;
  DeviceScope dev_scope(b->device);
  hipLaunchKernelGGL(p2p_receive_quality_kernel, dim3((b->S + 255) / 256), dim3(256), 0, b->stream, b->ts, rtt_ms,
                     frame_advantage, b->S, b->Spad, handle);
  RB_TRY(b, hipGetLastError());
  return RB_OK;
}

rb_status rb_p2p_export_time_sync(rb_p2p* b, int32_t* frames_ahead_dev, int32_t* local_adv_dev) {
  if (!b->ts_on) return fail(b, RB_INVALID_REQUEST, kTsOff);
  if (!frames_ahead_dev && !local_adv_dev) return RB_OK;
  DeviceScope dev_scope(b->device);
  hipLaunchKernelGGL(p2p_export_time_sync_kernel, dim3((b->S + 255) / 256), dim3(256), 0, b->stream, b->ts,
                     frames_ahead_dev, local_adv_dev, b->S, b->Spad, b->P);
  RB_TRY(b, hipGetLastError());
  return RB_OK;
}

rb_status rb_p2p_read_time_sync(rb_p2p* b, int32_t* frames_ahead, int32_t* local_adv, int32_t* remote_adv,
                                int32_t* rtt_ms) {
  if (!b->ts_on) return fail(b, RB_INVALID_REQUEST, kTsOff);
  DeviceScope dev_scope(b->device);
  std::vector<int32_t> st;
  rb_status r = read_rows(b, b->ts.state, TS_ROWS, st);
  if (r != RB_OK) return r;
  const size_t Sp = b->Spad;
  for (int s = 0; s < b->S; ++s) {
    if (frames_ahead) frames_ahead[s] = st[TS_FRAMES_AHEAD * Sp + s];
    for (int h = 0; h < b->P; ++h) {
      const size_t o = static_cast<size_t>(h) * b->S + s;
      if (local_adv) local_adv[o] = st[(TS_LOCAL_ADV + h) * Sp + s];
      if (remote_adv) remote_adv[o] = st[(TS_REMOTE_ADV + h) * Sp + s];
      if (rtt_ms) rtt_ms[o] = st[(TS_RTT + h) * Sp + s];
    }
  }
  return RB_OK;
}

rb_status rb_p2p_read_wait_recommendations(rb_p2p* b, uint32_t* counts, int32_t* frames, int32_t* skip_frames) {
  if (!b->ts_on) return fail(b, RB_INVALID_REQUEST, kTsOff);
  static_assert(kTsEvents == RB_P2P_WAIT_EVENTS_KEPT, "the event ring of time_sync.hpp");
  DeviceScope dev_scope(b->device);
  std::vector<int32_t> st;
  rb_status r = read_rows(b, b->ts.state, TS_ROWS, st);
  if (r != RB_OK) return r;
  const size_t Sp = b->Spad, E = kTsEvents;
  for (int s = 0; s < b->S; ++s) {
    const uint32_t cnt = static_cast<uint32_t>(st[TS_EV_N * Sp + s]), kept = cnt < E ? cnt : static_cast<uint32_t>(E);
    if (counts) counts[s] = cnt;
    for (size_t e = 0; e < E; ++e) {  // oldest kept first
      const bool has = e < kept;
      const size_t q = (cnt - kept + e) % E, o = static_cast<size_t>(s) * E + e;
      if (frames) frames[o] = has ? st[(TS_EV_FRAME + q) * Sp + s] : kNullFrame;
      if (skip_frames) skip_frames[o] = has ? st[(TS_EV_SKIP + q) * Sp + s] : 0;
    }
  }
  return RB_OK;
}

rb_status rb_p2p_debug_read_time_sync_windows(rb_p2p* b, int32_t* out) {
  if (!b->ts_on) return fail(b, RB_INVALID_REQUEST, kTsOff);
  DeviceScope dev_scope(b->device);
  std::vector<int32_t> w;
  rb_status r = read_rows(b, b->ts.win, 2 * static_cast<size_t>(kTsWindow) * 4, w);
  if (r != RB_OK) return r;
  for (int k = 0; k < 2; ++k)
    for (int i = 0; i < kTsWindow; ++i)
      for (int h = 0; h < b->P; ++h)
        for (int s = 0; s < b->S; ++s)
          out[((static_cast<size_t>(k) * kTsWindow + i) * b->P + h) * b->S + s] = w[ts_win_index(k, i, h, b->Spad, s)];
  return RB_OK;
}

rb_status rb_debug_time_sync_average(int32_t device, const int32_t* local_sums, const int32_t* remote_sums, int32_t* out,
                                     int64_t n) {
  if (n <= 0) return RB_OK;
  if (!local_sums || !remote_sums || !out) return RB_INVALID_REQUEST;
  if (device < 0) {
    for (int64_t i = 0; i < n; ++i) out[i] = time_sync_average(local_sums[i], remote_sums[i]);
    return RB_OK;
  }
  DeviceScope dev_scope(device);
  const size_t bytes = static_cast<size_t>(n) * 4;
  DeviceOwner tmp;  // freed on every return
  int32_t* d = nullptr;
  if (tmp.alloc(d, 3 * bytes) != hipSuccess) return RB_DEVICE_ERROR;
  if (hipMemcpy(d, local_sums, bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d + n, remote_sums, bytes, hipMemcpyHostToDevice) != hipSuccess)
    return RB_DEVICE_ERROR;
  hipLaunchKernelGGL(time_sync_average_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, nullptr, d,
                     d + n, d + 2 * n, n);
  const bool ok = hipGetLastError() == hipSuccess && hipMemcpy(out, d + 2 * n, bytes, hipMemcpyDeviceToHost) == hipSuccess;
  return ok ? RB_OK : RB_DEVICE_ERROR;
}

rb_status rb_p2p_read_desync_events(rb_p2p* b, uint32_t* counts, int32_t* frames, int32_t* handles,
                                    uint64_t* local_checksums, uint64_t* remote_checksums) {
  if (b->ds.interval <= 0) return fail(b, RB_INVALID_REQUEST, "desync detection is off (desync_interval = 0)");
  const size_t Sp = b->Spad, E = kEvents;
  std::vector<uint32_t> n;
  std::vector<int32_t> fr, hd;
  std::vector<uint64_t> lo, ro;
  rb_status r = read_rows(b, b->ds.ev_n, 1, n);
  if (r == RB_OK) r = read_rows(b, b->ds.ev_frame, E, fr);
  if (r == RB_OK) r = read_rows(b, b->ds.ev_handle, E, hd);
  if (r == RB_OK) r = read_rows(b, b->ds.ev_local, E, lo);
  if (r == RB_OK) r = read_rows(b, b->ds.ev_remote, E, ro);
  if (r != RB_OK) return r;
  for (int s = 0; s < b->S; ++s) {
    const uint32_t cnt = n[s], kept = cnt < E ? cnt : static_cast<uint32_t>(E);
    if (counts) counts[s] = cnt;
    for (size_t e = 0; e < E; ++e) {  // oldest kept first
      const bool has = e < kept;
      const size_t q = (cnt - kept + e) % E, o = static_cast<size_t>(s) * E + e;
      if (frames) frames[o] = has ? fr[q * Sp + s] : kNullFrame;
      if (handles) handles[o] = has ? hd[q * Sp + s] : -1;
      if (local_checksums) local_checksums[o] = has ? lo[q * Sp + s] : 0;
      if (remote_checksums) remote_checksums[o] = has ? ro[q * Sp + s] : 0;
    }
  }
  return RB_OK;
}

// ---- endpoint liveness (liveness.hpp)
rb_status rb_p2p_liveness_enable(rb_p2p* b, int32_t disconnect_timeout_ms, int32_t notify_start_ms) {
  if (b->lv_on) return fail(b, RB_INVALID_REQUEST, "rb_p2p_liveness_enable: liveness is already on");
  // disconnect_timeout - disconnect_notify_start is a Duration subtraction (protocol.rs:381): it panics below zero
  if (notify_start_ms < 0 || disconnect_timeout_ms < notify_start_ms)
    return fail(b, RB_INVALID_REQUEST, "rb_p2p_liveness_enable: needs 0 <= notify_start_ms <= disconnect_timeout_ms");
  DeviceScope dev_scope(b->device);
  if (const rb_status r = make_group(b, liveness_planes); r != RB_OK) return r;
  b->lv.timeout_ms = disconnect_timeout_ms;
  b->lv.notify_ms = notify_start_ms;
  b->lv_on = true;
  return RB_OK;
}

rb_status rb_p2p_poll_liveness(rb_p2p* b, int64_t now_ms, const uint8_t* received, const uint8_t* disconnect_requested,
                               uint8_t* state_out) {
  if (!b->lv_on) return fail(b, RB_INVALID_REQUEST, kLvOff);
  if (!received) return fail(b, RB_INVALID_REQUEST, "rb_p2p_poll_liveness: missing received tensor");
  if (now_ms < 0 || now_ms < b->lv_now)
    return fail(b, RB_INVALID_REQUEST, "rb_p2p_poll_liveness: now_ms is non-negative and never runs backwards");
  DeviceScope dev_scope(b->device);
  auto k = b->P == 2 ? p2p_liveness_kernel<2> : b->P == 3 ? p2p_liveness_kernel<3> : p2p_liveness_kernel<4>;
  hipLaunchKernelGGL(k, dim3((b->S + 255) / 256), dim3(256), 0, b->stream, b->lv, b->qs, b->status, received,
                     disconnect_requested, state_out, now_ms, b->cfg.local_mask, b->S, b->Spad);
  RB_TRY(b, hipGetLastError());
  b->lv_now = now_ms;
  b->mirror_stale = true;  // the timers disconnect players on the device
  return RB_OK;
}

rb_status rb_p2p_read_network_events(rb_p2p* b, uint32_t* counts, int32_t* kinds, int32_t* handles, int32_t* values) {
  if (!b->lv_on) return fail(b, RB_INVALID_REQUEST, kLvOff);
  static_assert(kLvEvents == RB_P2P_NET_EVENTS_KEPT, "the event ring of liveness.hpp");
  static_assert(kLvInterrupted == RB_NET_INTERRUPTED && kLvResumed == RB_NET_RESUMED && kLvDisconnected == RB_NET_DISCONNECTED,
                "the event kinds of liveness_step.hpp");
  DeviceScope dev_scope(b->device);
  const size_t Sp = b->Spad, E = kLvEvents;
  std::vector<uint32_t> n;
  std::vector<int32_t> ev;
  rb_status r = read_rows(b, b->lv.ev_n, 1, n);
  if (r == RB_OK) r = read_rows(b, b->lv.ev, LV_EV_ROWS * E, ev);
  if (r != RB_OK) return r;
  for (int s = 0; s < b->S; ++s) {
    const uint32_t cnt = n[s], kept = cnt < E ? cnt : static_cast<uint32_t>(E);
    if (counts) counts[s] = cnt;
    for (size_t e = 0; e < E; ++e) {  // oldest kept first
      const bool has = e < kept;
      const size_t q = (cnt - kept + e) % E, o = static_cast<size_t>(s) * E + e;
      if (kinds) kinds[o] = has ? ev[(LV_EV_KIND * E + q) * Sp + s] : 0;
      if (handles) handles[o] = has ? ev[(LV_EV_HANDLE * E + q) * Sp + s] : -1;
      if (values) values[o] = has ? ev[(LV_EV_VALUE * E + q) * Sp + s] : 0;
    }
  }
  return RB_OK;
}

rb_status rb_p2p_read_liveness(rb_p2p* b, int64_t* last_recv_ms, uint8_t* state) {
  if (!b->lv_on) return fail(b, RB_INVALID_REQUEST, kLvOff);
  DeviceScope dev_scope(b->device);
  std::vector<int64_t> st;
  std::vector<uint8_t> fl;
  std::vector<int32_t> misc;
  rb_status r = read_rows(b, b->lv.stamp, 4, st);
  if (r == RB_OK) r = read_rows(b, b->lv.flags, 4, fl);
  if (r == RB_OK) r = read_rows(b, b->qs + static_cast<size_t>(QS_PLAYER0 + QF_MISC * 4) * b->Spad, 4, misc);
  if (r != RB_OK) return r;
  for (int h = 0; h < b->P; ++h) {
    const bool local = (b->cfg.local_mask >> h) & 1u;
    for (int s = 0; s < b->S; ++s) {
      const size_t o = static_cast<size_t>(h) * b->S + s, c = static_cast<size_t>(h) * b->Spad + s;
      if (last_recv_ms) last_recv_ms[o] = local ? kLvUnstamped : st[c];
      if (state) state[o] = local ? 0 : static_cast<uint8_t>(fl[c] | ((static_cast<uint32_t>(misc[c]) & kQmDisc) ? 4u : 0u));
    }
  }
  return RB_OK;
}

rb_status rb_p2p_debug_corrupt(rb_p2p* b, int32_t session, int32_t word, uint32_t xor_mask) {
  if (session < 0 || session >= b->S || word < 0 || word >= b->ops->canon_words)
    return fail(b, RB_INVALID_REQUEST, "rb_p2p_debug_corrupt: session or word out of range");
  int lane = 0, w = 0;
  b->ops->word_loc(word, &lane, &w);
  const int L = b->ops->lanes, NW = b->ops->nw;
  const size_t idx = word_index(NW, b->Spad * L, session * L + lane, w);
  DeviceScope dev_scope(b->device);
  RB_TRY(b, hipStreamSynchronize(b->stream));
  const size_t plane = static_cast<size_t>(NW) * b->Spad * L;
  std::vector<uint32_t*> where{b->live + idx};
  for (int k = 0; k < b->W; ++k) where.push_back(b->snap + k * plane + idx);
  for (uint32_t* q : where) {
    uint32_t v = 0;
    RB_TRY(b, hipMemcpy(&v, q, 4, hipMemcpyDeviceToHost));
    v ^= xor_mask;
    RB_TRY(b, hipMemcpy(q, &v, 4, hipMemcpyHostToDevice));
  }
  return RB_OK;
}

rb_status rb_p2p_launch_clock_arm(rb_p2p* b, int32_t launches) {
  if (launches <= 0) return fail(b, RB_INVALID_REQUEST, "rb_p2p_launch_clock_arm: no launches");
  DeviceScope dev_scope(b->device);
  // one slot holds every wave of the widest launch of the batch: fanout_kernel's 16 branches per session
  const size_t lanes = static_cast<size_t>(b->Spad) * b->ops->lanes * (b->fanout ? kSpecBranches : 1);
  RB_TRY(b, b->clock.arm(b->res, launch_waves(lanes, b->block), static_cast<size_t>(launches), b->stream));
  return RB_OK;
}

rb_status rb_p2p_launch_clock_read(rb_p2p* b, uint64_t* start_end, int32_t cap, int32_t* launches) {
  if (!b->clock.armed) return fail(b, RB_INVALID_REQUEST, "rb_p2p_launch_clock_read: not armed");
  DeviceScope dev_scope(b->device);
  RB_TRY(b, b->clock.read(start_end, cap, launches, b->stream));
  return RB_OK;
}

rb_status rb_p2p_profile_enable(rb_p2p* b, int32_t on) {
  b->prof = on != 0;
  if (!b->prof) return RB_OK;
  DeviceScope dev_scope(b->device);
  RB_TRY(b, b->prof_ev.enable(b->stream));
  return RB_OK;
}

rb_status rb_p2p_profile_take(rb_p2p* b, double* total_ms, int32_t* launches) {
  RB_TRY(b, b->prof_ev.take(total_ms, nullptr, launches));
  return RB_OK;
}

}  // extern "C"
