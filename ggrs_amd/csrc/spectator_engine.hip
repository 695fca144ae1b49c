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
  uint32_t* tmpl = nullptr;             // the fresh columns restart_kernel copies (restart.hpp PlaneSet::tmpl)
  RestartIndex restart_idx;             // rb_spectator_restart_sessions' selected sessions
  RestartIndex move_idx;                // rb_spectator_export_sessions' / rb_spectator_import_sessions'
  uint32_t* refused = nullptr;          // [1] records rb_spectator_import_sessions refused since create
  std::string last_err;
};

namespace {
thread_local std::string g_spectator_err;

rb_status sfail(rb_spectator* b, rb_status st, const std::string& msg) {
  if (b) b->last_err = msg;
  else g_spectator_err = msg;
  return st;
}
#define SPT_TRY(b, expr)                                                                                    \
  do {                                                                                                      \
    hipError_t _e = (expr);                                                                                 \
    if (_e != hipSuccess) return sfail((b), RB_DEVICE_ERROR, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)

// hipSetDevice for the batch's calls, the caller's current device restored on every return
struct DeviceScope {
  int prev = -1;
  explicit DeviceScope(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

void free_all(rb_spectator* b) {
  (void)hipSetDevice(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  void* ptrs[] = {b->live, b->cs, b->frames, b->status, b->host, b->stats, b->counters, b->tmpl};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  b->restart_idx.release();
  b->move_idx.release();
  if (b->refused) (void)hipFree(b->refused);
  if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
}

template <class T>
rb_status read_rows(rb_spectator* b, const T* dev, size_t rows, std::vector<T>& host) {
  host.resize(rows * static_cast<size_t>(b->Spad));
  SPT_TRY(b, hipMemcpyAsync(host.data(), dev, host.size() * sizeof(T), hipMemcpyDeviceToHost, b->stream));
  SPT_TRY(b, hipStreamSynchronize(b->stream));
  return RB_OK;
}

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

// What a fresh spectator holds (restart.hpp): written into every column by rb_spectator_create and
// into the selected sessions' columns by rb_spectator_restart_sessions.  stats and counters are
// batch-wide.
void spectator_planes(const rb_spectator* b, PlaneSet& ps) {
  ps.Spad = static_cast<size_t>(b->Spad);
  const int NW = b->ops->nw, L = b->ops->lanes;
  std::vector<uint32_t> w0(static_cast<size_t>(L) * NW);
  b->ops->init_words(w0.data());
  ps.state(b->live, NW, L, 1, w0.data());  // State::new
  ps.fill(b->cs, b->ops->cs_bytes, 1, 1, 0);
  ps.fill(b->frames, 4, 2, 1, 0xff);        // current_frame, last_recv_frame: NULL_FRAME (:67-68)
  ps.row_values(b->status, 1, {0, -1});     // RB_OK; no tick yet
  ps.fill(b->host, 4, 4, 1, 0xff);          // ConnectionStatus::default: last_frame NULL_FRAME
  ps.fill(b->host + 4 * ps.Spad, 4, 4, 1, 0);  // connected
}
}  // namespace

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

const char* rb_spectator_last_error(const rb_spectator* b) { return b ? b->last_err.c_str() : g_spectator_err.c_str(); }

rb_status rb_spectator_create(const rb_spectator_config* cfg, rb_spectator** out) {
  *out = nullptr;
  if (!cfg || cfg->abi_version != RB_ABI_VERSION)
    return sfail(nullptr, RB_INVALID_REQUEST, "rb_spectator_config.abi_version mismatch");
  // builder.rs:210-244, on the final values.  They keep catchup_speed < max_frames_behind < 60,
  // which spectator_kernel relies on (spectator.hpp: both errors only on a tick's first frame).
  if (cfg->max_frames_behind < 1) return sfail(nullptr, RB_INVALID_REQUEST, "Max frames behind cannot be smaller than 1.");
  if (cfg->max_frames_behind >= kSpectatorBuffer)
    return sfail(nullptr, RB_INVALID_REQUEST,
                 "Max frames behind cannot be larger or equal than the Spectator buffer size (60)");
  if (cfg->catchup_speed < 1) return sfail(nullptr, RB_INVALID_REQUEST, "Catchup speed cannot be smaller than 1.");
  if (cfg->catchup_speed >= cfg->max_frames_behind)
    return sfail(nullptr, RB_INVALID_REQUEST,
                 "Catchup speed cannot be larger or equal than the allowed maximum frames behind host");
  static_assert(kSpectatorBuffer == 60, "the message above quotes SPECTATOR_BUFFER_SIZE");
  // the game and player-count rules of rb_p2p_create
  if (cfg->num_players <= 0 || cfg->num_players > 4 || cfg->num_sessions <= 0)
    return sfail(nullptr, RB_INVALID_REQUEST, "num_players must be 1..4; num_sessions positive");
  if (cfg->game != RB_GAME_EX_GAME && cfg->game != RB_GAME_STUB && cfg->game != RB_GAME_STUB_ENUM &&
      cfg->game != RB_GAME_BRAWLER && cfg->game < RB_GAME_PLUGIN_BASE)
    return sfail(nullptr, RB_INVALID_REQUEST,
                 "spectator batches support ex_game, the stub games, the brawler and registered plugin games");
  auto ops = make_game(cfg->game, cfg->num_players, false);
  if (!ops) return sfail(nullptr, RB_INVALID_REQUEST, "unsupported game / num_players combination");
  if (static_cast<uint64_t>(ops->nw) * ops->lanes * ((static_cast<uint64_t>(cfg->num_sessions) + 63) / 64 * 64) >= (1ull << 31))
    return sfail(nullptr, RB_INVALID_REQUEST, "batch too large for 31-bit state-plane offsets");
  // the input tensor's frame stride is 32-bit in the kernel
  if (static_cast<uint64_t>(cfg->num_players) * static_cast<uint64_t>(cfg->num_sessions) * ops->input_bytes >= (1ull << 32))
    return sfail(nullptr, RB_INVALID_REQUEST, "batch too large for a 32-bit input frame stride");

  auto b = std::make_unique<rb_spectator>();
  b->cfg = *cfg;
  b->ops = std::move(ops);
  b->S = cfg->num_sessions;
  b->Spad = (cfg->num_sessions + 63) / 64 * 64;
  b->P = cfg->num_players;
  b->block = cfg->block_size ? static_cast<int>(cfg->block_size) : 256;
  if (b->block % 64 != 0 || b->block > 256) return sfail(nullptr, RB_INVALID_REQUEST, "block_size must be 64, 128, 192 or 256");
  b->device = cfg->device;
  rb_spectator* bp = b.get();
  auto hip_fail = [&](hipError_t e, const char* what) {
    g_spectator_err = std::string(what) + ": " + hipGetErrorString(e);
    free_all(bp);
    return RB_DEVICE_ERROR;
  };
#define SPT_CREATE(expr)                              \
  do {                                                \
    hipError_t _e = (expr);                           \
    if (_e != hipSuccess) return hip_fail(_e, #expr); \
  } while (0)
  DeviceScope dev_scope(b->device);
  SPT_CREATE(hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking));
  b->stream = b->own_stream;
  const size_t Sp = b->Spad, NW = b->ops->nw, L = b->ops->lanes, Gp = Sp * L;
  SPT_CREATE(hipMalloc(&b->live, NW * Gp * 4));
  SPT_CREATE(hipMalloc(&b->cs, Sp * b->ops->cs_bytes));
  SPT_CREATE(hipMalloc(&b->frames, 2 * Sp * 4));
  SPT_CREATE(hipMalloc(&b->status, 2 * Sp * 4));
  SPT_CREATE(hipMalloc(&b->host, 8 * Sp * 4));
  SPT_CREATE(hipMalloc(&b->stats, SPT_COUNT * Sp * 8));
  SPT_CREATE(hipMalloc(&b->counters, 16));
  SPT_CREATE(hipMemsetAsync(b->stats, 0, SPT_COUNT * Sp * 8, b->stream));
  SPT_CREATE(hipMemsetAsync(b->counters, 0, 16, b->stream));
  // every session fresh: spectator_planes' values into every column, padding included
  PlaneSet ps;
  spectator_planes(bp, ps);
  SPT_CREATE(hipMalloc(&b->tmpl, ps.tmpl.size() * 4));
  SPT_CREATE(hipMemcpyAsync(b->tmpl, ps.tmpl.data(), ps.tmpl.size() * 4, hipMemcpyHostToDevice, b->stream));
  ps.bind(b->tmpl);
  SPT_CREATE(restart_launch(ps, nullptr, static_cast<uint32_t>(b->Spad), b->stream));
  SPT_CREATE(hipStreamSynchronize(b->stream));
#undef SPT_CREATE
  *out = b.release();
  return RB_OK;
}

void rb_spectator_destroy(rb_spectator* b) {
  if (!b) return;
  free_all(b);
  delete b;
}

rb_status rb_spectator_set_stream(rb_spectator* b, void* s) {
  SPT_TRY(b, hipStreamSynchronize(b->stream));
  b->stream = s ? static_cast<hipStream_t>(s) : b->own_stream;
  return RB_OK;
}

void* rb_spectator_get_stream(const rb_spectator* b) { return static_cast<void*>(b->stream); }

int32_t rb_spectator_state_bytes(const rb_spectator* b) { return b->ops->image_bytes; }
int32_t rb_spectator_input_bytes(const rb_spectator* b) { return b->ops->input_bytes; }

rb_status rb_spectator_receive_host_status(rb_spectator* b, const int32_t* last_frames, const uint8_t* disconnected) {
  if (!last_frames || !disconnected) return sfail(b, RB_INVALID_REQUEST, "missing connect-status tensor");
  DeviceScope dev_scope(b->device);
  hipLaunchKernelGGL(spectator_host_status_kernel, dim3((b->S + 255) / 256), dim3(256), 0, b->stream, b->host,
                     last_frames, disconnected, b->S, b->Spad, b->P);
  SPT_TRY(b, hipGetLastError());
  return RB_OK;
}

rb_status rb_spectator_restart_sessions(rb_spectator* b, const uint8_t* session_mask) {
  std::vector<int32_t> idx;
  if (session_mask) {
    restart_selected(session_mask, b->S, idx);
    if (idx.empty()) return RB_OK;
  }
  const bool all = !session_mask || idx.size() == static_cast<size_t>(b->S);
  DeviceScope dev_scope(b->device);
  PlaneSet ps;
  spectator_planes(b, ps);  // the same function, so the same template offsets, as at create
  ps.bind(b->tmpl);
  if (!all) SPT_TRY(b, b->restart_idx.upload(idx, static_cast<size_t>(b->S), b->stream));
  SPT_TRY(b, restart_launch(ps, all ? nullptr : b->restart_idx.dev, all ? static_cast<uint32_t>(b->S) : static_cast<uint32_t>(idx.size()),
                            b->stream));
  return RB_OK;
}

// ---- moving spectators between batches (migrate.hpp), as rb_p2p_export_sessions moves their hosts.
// Every plane of spectator_planes is carried: live state, checksum, frames, status, host status.
static RecordLayout record_planes(const rb_spectator* b, PlaneSet& ps) {
  ps.carry = true;
  spectator_planes(b, ps);
  const GameOps& o = *b->ops;
  return record_layout(plane_shapes(ps),
                       {2u /* a spectator batch */, static_cast<uint32_t>(b->cfg.game), static_cast<uint32_t>(b->P),
                        static_cast<uint32_t>(o.input_bytes), static_cast<uint32_t>(o.nw), static_cast<uint32_t>(o.lanes),
                        static_cast<uint32_t>(o.cs_bytes), static_cast<uint32_t>(o.image_bytes),
                        static_cast<uint32_t>(b->cfg.max_frames_behind), static_cast<uint32_t>(b->cfg.catchup_speed)});
}

static rb_status move_sessions(rb_spectator* b, const int32_t* sessions, int32_t n, void* records, bool scatter) {
  const char* const who = scatter ? "rb_spectator_import_sessions" : "rb_spectator_export_sessions";
  if (n < 0 || (n > 0 && (!sessions || !records))) return sfail(b, RB_INVALID_REQUEST, std::string(who) + ": missing session list or records");
  if (!move_indices_ok(sessions, n, b->S))
    return sfail(b, RB_INVALID_REQUEST, std::string(who) + ": sessions must be distinct indices in [0, num_sessions)");
  if (n == 0) return RB_OK;
  if (reinterpret_cast<uintptr_t>(records) % 16 != 0)
    return sfail(b, RB_INVALID_REQUEST, std::string(who) + ": records need 16-byte alignment");
  DeviceScope dev_scope(b->device);
  if (scatter && !b->refused) {
    SPT_TRY(b, hipMalloc(&b->refused, 4));
    SPT_TRY(b, hipMemsetAsync(b->refused, 0, 4, b->stream));
  }
  PlaneSet ps;
  const RecordLayout lay = record_planes(b, ps);
  SPT_TRY(b, b->move_idx.upload(std::vector<int32_t>(sessions, sessions + n), static_cast<size_t>(b->S), b->stream));
  SPT_TRY(b, move_launch(ps, lay, b->move_idx.dev, static_cast<uint32_t>(n), records, scatter, b->refused, b->stream));
  return RB_OK;
}

int64_t rb_spectator_session_record_bytes(const rb_spectator* b) {
  PlaneSet ps;
  return static_cast<int64_t>(record_planes(b, ps).record_bytes);
}

rb_status rb_spectator_export_sessions(rb_spectator* b, const int32_t* sessions, int32_t n, void* records_dev) {
  return move_sessions(b, sessions, n, records_dev, false);
}

rb_status rb_spectator_import_sessions(rb_spectator* b, const int32_t* sessions, int32_t n, const void* records_dev) {
  return move_sessions(b, sessions, n, const_cast<void*>(records_dev), true);
}

rb_status rb_spectator_import_refused(rb_spectator* b, uint32_t* count) {
  if (!count) return RB_OK;
  *count = 0;
  if (!b->refused) return RB_OK;  // no import yet
  DeviceScope dev_scope(b->device);
  SPT_TRY(b, hipMemcpyAsync(count, b->refused, 4, hipMemcpyDeviceToHost, b->stream));
  SPT_TRY(b, hipStreamSynchronize(b->stream));
  return RB_OK;
}

rb_status rb_spectator_run_ticks(rb_spectator* b, int32_t n_ticks, const int32_t* host_upto, const void* host_inputs,
                                 int32_t frames) {
  if (n_ticks <= 0) return RB_OK;
  if (!host_upto || !host_inputs || frames <= 0)
    return sfail(b, RB_INVALID_REQUEST, "rb_spectator_run_ticks: missing input tensor");
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
  p.in_frames = frames;
  p.S = b->S;
  p.Spad = b->Spad;
  p.T = n_ticks;
  p.max_behind = b->cfg.max_frames_behind;
  p.catchup = b->cfg.catchup_speed;
  DeviceScope dev_scope(b->device);
  const hipError_t e = b->ops->launch_spectator(p, b->block, b->stream);
  if (e != hipSuccess) return sfail(b, RB_DEVICE_ERROR, std::string("spectator launch: ") + hipGetErrorString(e));
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
  std::vector<int32_t> fr;
  std::vector<uint32_t> planes;
  rb_status r = read_rows(b, b->frames, 1, fr);
  if (r == RB_OK && images) r = read_rows(b, b->live, static_cast<size_t>(b->ops->nw) * b->ops->lanes, planes);
  if (r != RB_OK) return r;
  const int L = b->ops->lanes, NW = b->ops->nw;
  if (images) {
    std::vector<uint32_t> w(static_cast<size_t>(L) * NW);
    for (int s = 0; s < b->S; ++s) {
      for (int l = 0; l < L; ++l)
        for (int k = 0; k < NW; ++k) w[l * NW + k] = planes[word_index(NW, b->Spad * L, s * L + l, k)];
      b->ops->image(w.data(), fr[s] + 1, static_cast<uint8_t*>(images) + static_cast<size_t>(s) * b->ops->image_bytes);
    }
  }
  if (checksums) {
    std::vector<uint8_t> csh(static_cast<size_t>(b->Spad) * b->ops->cs_bytes);
    SPT_TRY(b, hipMemcpyAsync(csh.data(), b->cs, csh.size(), hipMemcpyDeviceToHost, b->stream));
    SPT_TRY(b, hipStreamSynchronize(b->stream));
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
