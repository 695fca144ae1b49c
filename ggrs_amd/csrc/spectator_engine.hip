// ggrs_amd/csrc/spectator_engine.hip — host side of the SpectatorSession batches
// (include/ggrs_amd.h rb_spectator_*): buffers, validation (builder.rs:210-244),
// launches of spectator_kernel (spectator.hpp) and the read-backs.
#include <cstring>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "migrate.hpp"

using namespace rb;

struct rb_spectator {
  rb_spectator_config cfg{};
  std::unique_ptr<GameOps> ops;
  int S = 0, Spad = 0, P = 0, block = 256;
  int device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  uint32_t* live = nullptr;
  void* cs = nullptr;
  int32_t* frames = nullptr;  // [2][Spad] current_frame, last_recv_frame
  int32_t* status = nullptr;  // [2][Spad] the last tick's rb_status, AdvanceFrame count
  int32_t* host = nullptr;    // [2][4][Spad] host_connect_status: last_frame, disconnected
  unsigned long long* stats = nullptr;  // [SPT_COUNT][Spad]
  uint32_t* counters = nullptr;         // [1] unexpected math paths
  uint32_t* tmpl = nullptr;             // the fresh columns restart_kernel copies (restart.hpp PlaneSet::tmpl), from create
  std::vector<uint32_t> tmpl_host;
  RestartIndex restart_idx;             // rb_spectator_restart_sessions' selected sessions
  RestartIndex move_idx;                // rb_spectator_export_sessions' / rb_spectator_import_sessions'
  uint32_t* refused = nullptr;          // [1] records rb_spectator_import_sessions refused since create
  int32_t ring_frames = 0;              // rb_spectator_set_delivery_ring: R, or 0 for a linear host_inputs (host state only)
  DeviceOwner res;                      // everything above that lies on the device
  std::string last_err;

  // what migrate.hpp's restart and move need of a batch
  static constexpr const char* kApi = "rb_spectator";
  void planes(PlaneSet& ps);
  std::vector<uint32_t> record_config() const;
  rb_status before_move() { return RB_OK; }
  ~rb_spectator() {
    if (!own_stream) return;  // nothing was made
    DeviceScope dev_scope(device);
    (void)hipStreamSynchronize(stream);
    res.release_all();
    (void)hipStreamDestroy(own_stream);
  }
};

namespace {
// UdpProtocol::on_input's connect-status merge (protocol.rs:629-636) into host_connect_status
__global__ void spectator_host_status_kernel(int32_t* __restrict__ host, const int32_t* __restrict__ last,
                                             const uint8_t* __restrict__ disc, int S, int Spad, int P) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  for (int i = 0; i < P; ++i) {
    const size_t o = static_cast<size_t>(i) * Spad + s, d = (4 + static_cast<size_t>(i)) * Spad + s;
    host[o] = max(host[o], last[static_cast<size_t>(i) * S + s]);
    host[d] = host[d] | (disc[static_cast<size_t>(i) * S + s] ? 1 : 0);
  }
}

}  // namespace

// What a fresh spectator holds, and the extent of each of its per-session buffers (restart.hpp):
// made and written into every column by rb_spectator_create, written into the selected sessions'
// columns by rb_spectator_restart_sessions, all of it carried by a move.  stats and counters are
// batch-wide.
void rb_spectator::planes(PlaneSet& ps) {
  rb_spectator* const b = this;
  const int NW = b->ops->nw, L = b->ops->lanes;
  std::vector<uint32_t> w0(static_cast<size_t>(L) * NW);
  b->ops->init_words(w0.data());
  ps.state(b->live, NW, L, 1, w0.data());  // State::new
  ps.fill(b->cs, b->ops->cs_bytes, 1, 1, 0);
  ps.fill(b->frames, 4, 2, 1, 0xff);        // current_frame, last_recv_frame: NULL_FRAME (:67-68)
  ps.row_values(b->status, 1, {0, -1});     // RB_OK; no tick yet
  ps.buffer(b->host, 4, 8, 1);
  ps.plane(b->host, 4, 4, 1, 0xff);          // ConnectionStatus::default: last_frame NULL_FRAME
  ps.plane(b->host + 4 * ps.Spad, 4, 4, 1, 0);  // connected
}
std::vector<uint32_t> rb_spectator::record_config() const {
  const GameOps& o = *ops;
  return {2u /* a spectator batch */, static_cast<uint32_t>(cfg.game), static_cast<uint32_t>(P),
          static_cast<uint32_t>(o.input_bytes), static_cast<uint32_t>(o.nw), static_cast<uint32_t>(o.lanes),
          static_cast<uint32_t>(o.cs_bytes), static_cast<uint32_t>(o.image_bytes),
          static_cast<uint32_t>(cfg.max_frames_behind), static_cast<uint32_t>(cfg.catchup_speed)};
}

extern "C" {

void rb_spectator_config_init(rb_spectator_config* c) {
  std::memset(c, 0, sizeof(*c));
  c->abi_version = RB_ABI_VERSION;
  c->game = RB_GAME_EX_GAME;
  c->num_sessions = 1;
  c->num_players = 2;         // builder.rs:13
  c->device = 0;
  c->max_frames_behind = 10;  // builder.rs:23
  c->catchup_speed = 1;       // builder.rs:25
}

const char* rb_spectator_last_error(const rb_spectator* b) { return b ? b->last_err.c_str() : g_create_err.c_str(); }

rb_status rb_spectator_create(const rb_spectator_config* cfg, rb_spectator** out) {
  *out = nullptr;
  if (!cfg || cfg->abi_version != RB_ABI_VERSION)
    return fail(nullptr, RB_INVALID_REQUEST, "rb_spectator_config.abi_version mismatch");
  // builder.rs:210-244, on the final values.  They keep catchup_speed < max_frames_behind < 60,
  // which spectator_kernel relies on (spectator.hpp: both errors only on a tick's first frame).
  if (cfg->max_frames_behind < 1) return fail(nullptr, RB_INVALID_REQUEST, "Max frames behind cannot be smaller than 1.");
  if (cfg->max_frames_behind >= kSpectatorBuffer)
    return fail(nullptr, RB_INVALID_REQUEST,
                "Max frames behind cannot be larger or equal than the Spectator buffer size (60)");
  if (cfg->catchup_speed < 1) return fail(nullptr, RB_INVALID_REQUEST, "Catchup speed cannot be smaller than 1.");
  if (cfg->catchup_speed >= cfg->max_frames_behind)
    return fail(nullptr, RB_INVALID_REQUEST,
                "Catchup speed cannot be larger or equal than the allowed maximum frames behind host");
  static_assert(kSpectatorBuffer == 60, "the message above quotes SPECTATOR_BUFFER_SIZE");
  // the game and player-count rules of rb_p2p_create
  if (cfg->num_players <= 0 || cfg->num_players > 4 || cfg->num_sessions <= 0)
    return fail(nullptr, RB_INVALID_REQUEST, "num_players must be 1..4; num_sessions positive");
  if (cfg->game != RB_GAME_EX_GAME && cfg->game != RB_GAME_STUB && cfg->game != RB_GAME_STUB_ENUM &&
      cfg->game != RB_GAME_BRAWLER && cfg->game < RB_GAME_PLUGIN_BASE)
    return fail(nullptr, RB_INVALID_REQUEST,
                "spectator batches support ex_game, the stub games, the brawler and registered plugin games");
  auto ops = make_game(cfg->game, cfg->num_players, false);
  if (!ops) return fail(nullptr, RB_INVALID_REQUEST, "unsupported game / num_players combination");
  if (static_cast<uint64_t>(ops->nw) * ops->lanes * ((static_cast<uint64_t>(cfg->num_sessions) + 63) / 64 * 64) >= (1ull << 31))
    return fail(nullptr, RB_INVALID_REQUEST, "batch too large for 31-bit state-plane offsets");
  // the input tensor's frame stride is 32-bit in the kernel
  if (static_cast<uint64_t>(cfg->num_players) * static_cast<uint64_t>(cfg->num_sessions) * ops->input_bytes >= (1ull << 32))
    return fail(nullptr, RB_INVALID_REQUEST, "batch too large for a 32-bit input frame stride");

  auto b = std::make_unique<rb_spectator>();
  b->cfg = *cfg;
  b->ops = std::move(ops);
  b->S = cfg->num_sessions;
  b->Spad = (cfg->num_sessions + 63) / 64 * 64;
  b->P = cfg->num_players;
  b->block = cfg->block_size ? static_cast<int>(cfg->block_size) : 256;
  if (b->block % 64 != 0 || b->block > 256) return fail(nullptr, RB_INVALID_REQUEST, "block_size must be 64, 128, 192 or 256");
  b->device = cfg->device;
  // a failure from here on frees what was made (~rb_spectator) and leaves its message for rb_spectator_last_error(nullptr)
  DeviceScope dev_scope(b->device);
  RB_TRY(nullptr, hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking));
  b->stream = b->own_stream;
  const size_t Sp = b->Spad;
  RB_TRY(nullptr, b->res.alloc(b->stats, SPT_COUNT * Sp * 8));
  RB_TRY(nullptr, b->res.alloc(b->counters, 16));
  RB_TRY(nullptr, hipMemsetAsync(b->stats, 0, SPT_COUNT * Sp * 8, b->stream));
  RB_TRY(nullptr, hipMemsetAsync(b->counters, 0, 16, b->stream));
  // every session fresh: the planes' buffers made, their values into every column, padding included
  PlaneSet ps;
  ps.Spad = Sp;
  ps.make = &b->res;
  b->planes(ps);
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

void rb_spectator_destroy(rb_spectator* b) { delete b; }

rb_status rb_spectator_set_stream(rb_spectator* b, void* s) {
  RB_TRY(b, hipStreamSynchronize(b->stream));
  b->stream = s ? static_cast<hipStream_t>(s) : b->own_stream;
  return RB_OK;
}

void* rb_spectator_get_stream(const rb_spectator* b) { return static_cast<void*>(b->stream); }

int32_t rb_spectator_state_bytes(const rb_spectator* b) { return b->ops->image_bytes; }
int32_t rb_spectator_input_bytes(const rb_spectator* b) { return b->ops->input_bytes; }

rb_status rb_spectator_receive_host_status(rb_spectator* b, const int32_t* last_frames, const uint8_t* disconnected) {
  if (!last_frames || !disconnected) return fail(b, RB_INVALID_REQUEST, "missing connect-status tensor");
  DeviceScope dev_scope(b->device);
  hipLaunchKernelGGL(spectator_host_status_kernel, dim3((b->S + 255) / 256), dim3(256), 0, b->stream, b->host,
                     last_frames, disconnected, b->S, b->Spad, b->P);
  RB_TRY(b, hipGetLastError());
  return RB_OK;
}

rb_status rb_spectator_restart_sessions(rb_spectator* b, const uint8_t* session_mask) {
  std::vector<int32_t> idx;
  return restart_sessions(b, session_mask, idx);
}

// ---- moving spectators between batches (migrate.hpp), as rb_p2p_export_sessions moves their hosts.
// Every plane of rb_spectator::planes is carried: live state, checksum, frames, status, host status.
int64_t rb_spectator_session_record_bytes(const rb_spectator* b) {
  PlaneSet ps;  // (layout only: nothing of the batch is written)
  return static_cast<int64_t>(record_planes(const_cast<rb_spectator*>(b), ps, true).record_bytes);
}

rb_status rb_spectator_export_sessions(rb_spectator* b, const int32_t* sessions, int32_t n, void* records_dev) {
  return move_sessions(b, sessions, n, records_dev, false);
}

rb_status rb_spectator_import_sessions(rb_spectator* b, const int32_t* sessions, int32_t n, const void* records_dev) {
  return move_sessions(b, sessions, n, const_cast<void*>(records_dev), true);
}

rb_status rb_spectator_import_refused(rb_spectator* b, uint32_t* count) { return import_refused(b, count); }

rb_status rb_spectator_run_ticks(rb_spectator* b, int32_t n_ticks, const int32_t* host_upto, const void* host_inputs,
                                 int32_t frames) {
  if (n_ticks <= 0) return RB_OK;
  if (!host_upto || !host_inputs || frames <= 0)
    return fail(b, RB_INVALID_REQUEST, "rb_spectator_run_ticks: missing input tensor");
  if (b->ring_frames && frames != b->ring_frames)
    return fail(b, RB_INVALID_REQUEST,
                "the batch has a delivery ring (rb_spectator_set_delivery_ring): host_inputs holds exactly ring_frames frames");
  SpectatorParams p{};
  p.live = b->live;
  p.cs = b->cs;
  p.frames = b->frames;
  p.status = b->status;
  p.host_last = b->host;
  p.host_disc = b->host + 4 * static_cast<size_t>(b->Spad);
  p.stats = b->stats;
  p.counters = b->counters;
  p.upto = host_upto;
  p.in = static_cast<const uint8_t*>(host_inputs);
  // a delivery ring: no frame is clamped to the tensor's length, frame f sits in slot f & (R - 1)
  p.in_frames = b->ring_frames ? INT32_MAX : frames;
  p.in_mask = b->ring_frames ? b->ring_frames - 1 : INT32_MAX;
  p.S = b->S;
  p.Spad = b->Spad;
  p.T = n_ticks;
  p.max_behind = b->cfg.max_frames_behind;
  p.catchup = b->cfg.catchup_speed;
  DeviceScope dev_scope(b->device);
  const hipError_t e = b->ops->launch_spectator(p, b->block, b->stream);
  if (e != hipSuccess) return fail(b, RB_DEVICE_ERROR, std::string("spectator launch: ") + hipGetErrorString(e));
  return RB_OK;
}

rb_status rb_spectator_set_delivery_ring(rb_spectator* b, int32_t ring_frames) {
  if (ring_frames != 0 && (ring_frames < RB_INPUT_QUEUE_LENGTH || (ring_frames & (ring_frames - 1)) != 0))
    return fail(b, RB_INVALID_REQUEST, "rb_spectator_set_delivery_ring: ring_frames is 0 or a power of two of at least 128");
  if (ring_frames != 0 && b->cfg.game >= RB_GAME_PLUGIN_BASE && !plugin_masks_delivery_frames(b->cfg.game))
    return fail(b, RB_INVALID_REQUEST, "rb_spectator_set_delivery_ring: rebuild the game plugin against the current headers");
  b->ring_frames = ring_frames;
  return RB_OK;
}

rb_status rb_spectator_read_status(rb_spectator* b, int32_t* status, int32_t* n_advance) {
  std::vector<int32_t> st;
  rb_status r = read_rows(b, b->status, 2, st);
  if (r != RB_OK) return r;
  for (int s = 0; s < b->S; ++s) {
    if (status) status[s] = st[s];
    if (n_advance) n_advance[s] = st[static_cast<size_t>(b->Spad) + s];
  }
  return RB_OK;
}

rb_status rb_spectator_read_frames(rb_spectator* b, int32_t* current, int32_t* last_recv) {
  std::vector<int32_t> fr;
  rb_status r = read_rows(b, b->frames, 2, fr);
  if (r != RB_OK) return r;
  for (int s = 0; s < b->S; ++s) {
    if (current) current[s] = fr[s];
    if (last_recv) last_recv[s] = fr[static_cast<size_t>(b->Spad) + s];
  }
  return RB_OK;
}

rb_status rb_spectator_read_live(rb_spectator* b, void* images, uint64_t* checksums) {
  DeviceScope dev_scope(b->device);
  std::vector<int32_t> fr;
  std::vector<uint32_t> planes;
  rb_status r = read_rows(b, b->frames, 1, fr);
  if (r == RB_OK && images) r = read_rows(b, b->live, static_cast<size_t>(b->ops->nw) * b->ops->lanes, planes);
  if (r != RB_OK) return r;
  const int L = b->ops->lanes, NW = b->ops->nw;
  if (images) {
    std::vector<uint32_t> w(static_cast<size_t>(L) * NW);
    for (int s = 0; s < b->S; ++s) {
      session_words(planes.data(), NW, L, b->Spad, s, w.data());
      b->ops->image(w.data(), fr[s] + 1, static_cast<uint8_t*>(images) + static_cast<size_t>(s) * b->ops->image_bytes);
    }
  }
  if (checksums) {
    std::vector<uint8_t> csh(static_cast<size_t>(b->Spad) * b->ops->cs_bytes);
    RB_TRY(b, hipMemcpyAsync(csh.data(), b->cs, csh.size(), hipMemcpyDeviceToHost, b->stream));
    RB_TRY(b, hipStreamSynchronize(b->stream));
    for (int s = 0; s < b->S; ++s) {
      const U128 c = b->ops->cs_at(csh.data(), static_cast<size_t>(s));
      checksums[static_cast<size_t>(s) * 2] = c.lo;
      checksums[static_cast<size_t>(s) * 2 + 1] = c.hi;
    }
  }
  return RB_OK;
}

rb_status rb_spectator_totals(rb_spectator* b, uint64_t* out3) {
  std::vector<unsigned long long> st;
  rb_status r = read_rows(b, b->stats, SPT_COUNT, st);
  if (r != RB_OK) return r;
  for (int i = 0; i < SPT_COUNT; ++i) {
    uint64_t t = 0;
    for (int s = 0; s < b->S; ++s) t += st[static_cast<size_t>(i) * b->Spad + s];
    out3[i] = t;
  }
  return RB_OK;
}

}  // extern "C"
