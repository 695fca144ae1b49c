/* ===========================================================================
 * ggrs_amd.h — C ABI of the MI355X batched rollback-resimulation engine.
 *
 * Drop-in boundary for the GGRS 0.9.4 resimulation path (/root/reference):
 * a batch of S lock-step SyncTestSessions whose request stream
 * (SaveGameState / LoadGameState / AdvanceFrame, lib.rs:170-194) is produced
 * by host-side bookkeeping identical to the reference and executed on the GPU
 * by compiled-in game handlers (the user's `handle_requests`, ex_game.rs:76-84).
 *
 * Plain C types only (no torch, no HIP types in signatures): a Rust `extern
 * "C"` block, a ctypes stub or a C++ wrapper binds it directly; see
 * INTEGRATION.md.  Every entry point names the reference interface it
 * replaces.
 *
 * Threading: one batch = one HIP stream; calls on one batch are not reentrant.
 * Different batches (e.g. one per GPU) may be driven from different threads.
 * No exception or panic crosses the ABI: every call returns rb_status.
 * ======================================================================== */
#ifndef GGRS_AMD_H
#define GGRS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RB_ABI_VERSION 1
#define RB_NULL_FRAME (-1) /* lib.rs:46 NULL_FRAME */
#define RB_INPUT_QUEUE_LENGTH 128 /* input_queue.rs:6 */

/* GGRSError (error.rs:11-36) as status codes, plus engine-side failures. */
typedef enum rb_status {
  RB_OK = 0,
  RB_PREDICTION_THRESHOLD = 1,     /* GGRSError::PredictionThreshold          error.rs:13 */
  RB_INVALID_REQUEST = 2,          /* GGRSError::InvalidRequest{info}         error.rs:15-18 (info: rb_last_error) */
  RB_MISMATCHED_CHECKSUM = 3,      /* GGRSError::MismatchedChecksum{frame}    error.rs:22-25 (per session: rb_mismatches) */
  RB_NOT_SYNCHRONIZED = 4,         /* GGRSError::NotSynchronized              error.rs:27 */
  RB_SPECTATOR_TOO_FAR_BEHIND = 5, /* GGRSError::SpectatorTooFarBehind        error.rs:29 */
  RB_DEVICE_ERROR = 100,           /* HIP runtime failure (no reference analogue) */
  RB_PANIC = 101                   /* a reference assert!/panic! condition was hit (API misuse) */
} rb_status;

/* Compiled-in game handlers (the `Config` trait's State/Input + handle_requests).
 * Input domain: every value of the input type is a legal input, as in the reference
 * (its inputs are Pod).  ex_game's State::advance reads bits 0-3 of its byte, while the
 * InputQueue compares, predicts and ships the whole byte: SyncTest, P2P (plain, sparse,
 * every fan-out form, packet-fed), spectators and the brawler's fan-out are tested over
 * all 256 byte values, the stub game over any u32 (tests/test_input_domain.py,
 * tests/test_wire_edges.py). */
typedef enum rb_game {
  RB_GAME_EX_GAME = 1,        /* examples/ex_game/ex_game.rs: f32 ships, Input{inp:u8}, fletcher16 over the bincode image */
  RB_GAME_STUB = 2,           /* tests/stubs.rs GameStub: i32 state, StubInput{inp:u32}, SipHash-1-3 checksum */
  RB_GAME_STUB_ENUM = 3,      /* tests/stubs_enum.rs GameStubEnum: #[repr(u8)] enum input */
  RB_GAME_STUB_RANDOM_CS = 4, /* tests/stubs.rs RandomChecksumGameStub: random u128 checksums (forces mismatches) */
  RB_GAME_BRAWLER = 5         /* BASELINE config 3: fixed-point 256-entity brawler, 8 KiB state, Input{inp:u8}, fletcher16;
                                 no reference game exists: defined in oracle/ggrs_oracle.hpp */
} rb_game;

/* Games compiled outside the engine (include/ggrs_amd_game.hpp: the `Config`
 * trait + handle_requests of the user's game as device code, built into a
 * plugin library by ggrs_amd/csrc/plugin.hip).  rb_register_game_plugin
 * loads one and returns its game id (RB_GAME_PLUGIN_BASE + k), valid for
 * rb_config.game and rb_p2p_config.game from then on.  Registering the same
 * path twice returns the same id.  RB_INVALID_REQUEST: the library cannot be
 * loaded, lacks the entry points or was built for another plugin ABI. */
#define RB_GAME_PLUGIN_BASE 1000
rb_status rb_register_game_plugin(const char* path, int32_t* game_id);

/* GGRSRequest kinds (lib.rs:170-194) for rb_last_requests. */
typedef enum rb_request_kind { RB_REQ_SAVE = 0, RB_REQ_LOAD = 1, RB_REQ_ADVANCE = 2 } rb_request_kind;

#define RB_FLAG_CHECKED 1u          /* advance_frame reports MismatchedChecksum synchronously, like the reference (default) */
#define RB_FLAG_LANE_PER_SESSION 2u /* ex_game: one lane per session instead of one lane per player; only
                                       libraries built with RB_EXPERIMENTS=1 accept it (the product library
                                       refuses it at create with RB_INVALID_REQUEST) */

/* SessionBuilder fields used by start_synctest_session (builder.rs:32-52). */
typedef struct rb_config {
  int32_t abi_version;    /* = RB_ABI_VERSION */
  int32_t game;           /* rb_game */
  int32_t num_sessions;   /* batch size S (independent sessions in lock-step) */
  int32_t num_players;    /* with_num_players          builder.rs:154-157 (default 2) */
  int32_t max_prediction; /* with_max_prediction_window builder.rs:136-145 (default 8, >0, <= 64 here) */
  int32_t check_distance; /* with_check_distance       builder.rs:202-205 (default 2, < max_prediction) */
  int32_t input_delay;    /* with_input_delay          builder.rs:148-151 (default 0) */
  int32_t device;         /* HIP device ordinal; -1 = plan-only batch (host bookkeeping, no device work) */
  uint64_t seed;          /* RB_GAME_STUB_RANDOM_CS only */
  uint32_t flags;         /* RB_FLAG_* */
  uint32_t block_size;    /* 0 = default; kernel tuning knob */
  uint32_t reserved[6];
} rb_config;

typedef struct rb_batch rb_batch;

/* Checksum report record (mirrors messages.rs:75-79 ChecksumReport{checksum:u128, frame}
 * + the session's desync flag) written to device memory by rb_export_checksum_report. */
typedef struct rb_checksum_report {
  uint64_t checksum_lo;
  uint64_t checksum_hi;
  int32_t frame;
  int32_t mismatch_frame; /* RB_NULL_FRAME when the session is healthy */
} rb_checksum_report;

/* SessionBuilder::new() defaults (builder.rs:13-27, 62-78). */
void rb_config_init(rb_config* cfg);

/* SessionBuilder::start_synctest_session (builder.rs:342-354) for S sessions.
 * Validation errors as in the reference ("Check distance too big.", zero
 * prediction window) -> RB_INVALID_REQUEST; *out = NULL and the message via
 * rb_last_error(NULL). */
rb_status rb_synctest_create(const rb_config* cfg, rb_batch** out);
void rb_destroy(rb_batch* b);

/* Last error message of this batch (or of the failed create when b == NULL). */
const char* rb_last_error(const rb_batch* b);

/* Run this batch on a caller-owned hipStream_t (passed as void*); NULL = the
 * batch's own stream. */
rb_status rb_set_stream(rb_batch* b, void* hip_stream);
/* The hipStream_t the batch runs on (its own one unless rb_set_stream chose
 * another); NULL for a plan-only batch.  Callers order their own streams
 * against it (ggrs_amd/session.py _StreamOrdered). */
void* rb_get_stream(const rb_batch* b);

/* SyncTestSession::add_local_input (sync_test_session.rs:61-74) for every
 * session at once: `inputs` holds S values of the game's Input type
 * (ex_game: u8, stub: u32, enum: u8) for player `handle`; host or device
 * pointer.  Device pointers must stay valid until the next advance has run
 * (stream order).  Overwrites an earlier call for the same handle.
 * handle >= num_players -> RB_INVALID_REQUEST. */
rb_status rb_add_local_input(rb_batch* b, int32_t handle, const void* inputs, int32_t on_device);

/* All players at once, packed [S][num_players] Input values. */
rb_status rb_add_local_inputs_packed(rb_batch* b, const void* inputs, int32_t on_device);

/* SyncTestSession::advance_frame (sync_test_session.rs:85-146) followed by
 * the game's handle_requests on every session, fused into one device launch.
 * Returns RB_INVALID_REQUEST (missing input), RB_PREDICTION_THRESHOLD, or —
 * with RB_FLAG_CHECKED — RB_MISMATCHED_CHECKSUM when at least one session's
 * advance_frame returned Err(MismatchedChecksum) in this call.  A session that
 * failed does not advance (as in the reference, where every retry fails the
 * same way); the others do.  Without RB_FLAG_CHECKED the call is fully
 * asynchronous and mismatches are read with rb_mismatches. */
rb_status rb_advance_frame(rb_batch* b);

/* n_ticks x (add_local_input for every handle + advance_frame) in one call:
 * tick t reads its inputs at inputs + t*tick_stride_bytes, laid out
 * [num_players][num_sessions] Input values (host or device memory).  The host
 * bookkeeping runs tick by tick as in rb_advance_frame; consecutive
 * steady-state ticks (current frame > check_distance, 1 <= check_distance <= 16)
 * execute as ONE fused device launch (for games of at most 80 B of state per
 * cell, e.g. ex_game and the stubs, while the batch's snapshot ring is below
 * 4 GiB: ex_game P=2, W=8 holds 40 B per session per slot, 320 B per session,
 * so up to 13.4M sessions; larger rings run one launch per tick, same results).  A session whose resimulation
 * mismatches stops advancing (as with per-tick calls) while the others run
 * on; with RB_FLAG_CHECKED the call returns RB_MISMATCHED_CHECKSUM if any
 * session has failed by its end.  Bookkeeping errors (RB_INVALID_REQUEST,
 * RB_PREDICTION_THRESHOLD, RB_PANIC) stop the run; *ticks_done = completed ticks. */
rb_status rb_run_ticks(rb_batch* b, int32_t n_ticks, const void* inputs, int64_t tick_stride_bytes,
                       int32_t on_device, int32_t* ticks_done);

/* SyncLayer::current_frame of the batch (sync_layer.rs:110-112). */
int32_t rb_current_frame(const rb_batch* b);
int32_t rb_num_sessions(const rb_batch* b);
/* Bytes of one session's canonical state image (ex_game: the bincode image,
 * 36+20*P; stubs: le32 frame || le32 state) and of one Input value. */
int32_t rb_state_bytes(const rb_batch* b);
int32_t rb_input_bytes(const rb_batch* b);

/* Wait for all work queued on the batch's stream. */
rb_status rb_synchronize(rb_batch* b);

/* Per-session MismatchedChecksum{frame} (RB_NULL_FRAME when healthy) and the
 * count of failed sessions.  Synchronises. */
rb_status rb_mismatches(rb_batch* b, int32_t* frames_out, int32_t* count_out);

/* The (kind, frame) list of the request stream the last rb_advance_frame
 * executed, identical to the Vec<GGRSRequest> the reference returns
 * (AdvanceFrame carries the frame it advances from).  Returns the count. */
int32_t rb_last_requests(const rb_batch* b, int32_t* kinds, int32_t* frames, int32_t cap);

/* GameStateCell::{load, checksum} (sync_layer.rs:28-39) for the cell holding
 * `frame`: images [S][rb_state_bytes], checksums [S][2] (u128 lo, hi).
 * RB_INVALID_REQUEST if no cell holds that frame.  Synchronises. */
rb_status rb_read_cell(rb_batch* b, int32_t frame, void* images, uint64_t* checksums);

/* The game's live state after the last advance (ex_game Game::game_state,
 * images [S][rb_state_bytes]) and its display checksum with its frame
 * (Game::last_checksum, ex_game.rs:104-111; [S] each; RB_NULL_FRAME for games
 * without one).  A failed session reports the state it stopped at.  Synchronises. */
rb_status rb_read_live(rb_batch* b, void* images, uint64_t* display_checksums, int32_t* display_frames);

/* Desync report for the cell holding `frame` into device memory [S]
 * rb_checksum_report (the P2P ChecksumReport payload; multi-GPU allgather
 * input).  Stream-ordered, does not synchronise. */
rb_status rb_export_checksum_report(rb_batch* b, int32_t frame, void* dev_out);

/* The same report in 4 bytes per session, for games whose checksum is 16 bits
 * (ex_game's fletcher16): dev_out[S] uint32 records
 *   bits 0-15   the checksum of the cell holding `frame` (ChecksumReport::checksum)
 *   bits 16-30  frame - mismatch_frame, saturated at 0x7FFF (0 when healthy)
 *   bit  31     the session reports MismatchedChecksum
 * The report frame (ChecksumReport::frame, messages.rs:75-79) is batch-uniform in
 * SyncTest, so it travels once per all-gather instead of once per session: the
 * multi-GPU gather moves 4 B per session instead of 24.  RB_INVALID_REQUEST for a
 * game with a wider checksum (use rb_export_checksum_report).  Stream-ordered. */
rb_status rb_export_compact_report(rb_batch* b, int32_t frame, void* dev_out);

/* Fault injection for tests: XOR `xor_mask` into state word `word` of
 * `session` in the cell holding `frame` (a corrupted snapshot makes the next
 * resimulation diverge, which SyncTest must report). */
rb_status rb_debug_corrupt_cell(rb_batch* b, int32_t session, int32_t frame, int32_t word, uint32_t xor_mask);

/* Device evaluation of the game's sin/cos (the glibc sinf/cosf restatement in
 * device_math.hpp) for n host floats, on `device` — pins it against the host
 * libm in the parity tests. */
rb_status rb_debug_sincosf(int32_t device, const float* x, float* sin_out, float* cos_out, int64_t n);

/* The in-range forms of the same arithmetic the fused steady ticks and the fan-out run
 * (sincosf_glibc<true>, and the rotation step rem_euclid(x +- ROTATION_SPEED, 2 pi),
 * ex_game.rs:282-296, as rem_euclid_near<true> and rem_euclid<true>) for the n floats whose
 * bits are first_bits, first_bits + 1, ... (all in [+0, 6.5)), into device memory dev_out
 * [6][n] (sin, cos, step up, step down, step up, step down).  Synchronises. */
rb_status rb_debug_exgame_inrange(int32_t device, uint32_t first_bits, int64_t n, float* dev_out);

/* ex_game's position clamp x.max(0).min(L) (ex_game.rs:311-314) as the fused steady ticks run it,
 * one median of three, against the two-step form, both evaluated on the device for the n floats
 * whose bits are first_bits, first_bits + 1, ... (first_bits + n <= 2^32) and for both limits
 * (600 and 800).  diff[0] (host) = the number of patterns whose two forms differ in any bit,
 * diff[1] = the smallest such pattern (all ones when none); signalling NaNs (0x7F800001-0x7FBFFFFF,
 * 0xFF800001-0xFFBFFFFF) are left out: a position is the result of an f32 add.  dev_out: null, or
 * device memory [2][n] for the one-instruction form's results (L = 600, L = 800).  Synchronises. */
rb_status rb_debug_exgame_position_clamp(int32_t device, uint32_t first_bits, int64_t n, uint64_t* diff, float* dev_out);

/* Device evaluation of ex_game's speed clamp (ex_game.rs:300-304: v * MAX_SPEED
 * / |v| when |v| > MAX_SPEED) for n host (vx, vy) pairs — pins the short exact
 * sqrt/division sequences of device_math.hpp against host IEEE arithmetic. */
rb_status rb_debug_speed_clamp(int32_t device, const float* vx, const float* vy, float* vx_out, float* vy_out,
                               int64_t n);

/* HIP event timing of the tick kernel on the batch's stream, for bench.py:
 * rb_profile_enable(b, k) brackets every k-th single-tick launch (k <= 1:
 * every 8th) and every fused rb_run_ticks launch with an event pair;
 * rb_profile_take returns the summed milliseconds of the timed launches and
 * the number of ticks they covered, and resets both. */
rb_status rb_profile_enable(rb_batch* b, int32_t on);
rb_status rb_profile_take(rb_batch* b, double* total_ms, int32_t* launches);

/* The kernel's own clock (measurement only, no reference counterpart: bench.py's
 * kernel time).  rb_launch_clock_arm(b, n): the next n fused steady launches
 * (rb_run_ticks) have every wave store its start and end on the chip's 100 MHz
 * constant clock into a slot of their own (cleared here, once: nothing is added
 * to the launches' stream).  rb_launch_clock_read(b, out[2 * cap], cap, &n)
 * waits for the stream, returns per launch the first wave's start and the last
 * wave's end in 10 ns ticks, and disarms.  No host call or event sits between
 * the two readings and a profiler does not change them; the dispatch's own
 * setup and end-of-kernel release fall outside them (bench.py adds the
 * calibrated difference to rocprofv3's dispatch duration). */
rb_status rb_launch_clock_arm(rb_batch* b, int32_t launches);
rb_status rb_launch_clock_read(rb_batch* b, uint64_t* start_end, int32_t cap, int32_t* launches);

/* ===========================================================================
 * P2PSession batches (sessions/p2p_session.rs) — the rollback path.
 *
 * S independent P2P sessions seen from one peer, each with num_players
 * handles: bit h of local_mask set = add_player(PlayerType::Local, h), clear =
 * PlayerType::Remote (builder.rs:90-128).  The network layer is not part of
 * the batch: UdpProtocol's role on this path, turning packets into
 * Event::Input{input, player} in frame order (p2p_session.rs:838-852), is the
 * caller's: per tick and remote handle it passes the newest delivered frame
 * (`remote_upto`) and the inputs by frame (`remote_inputs`).  Mispredicted
 * remote inputs roll sessions back individually (per-session depth), on the
 * device.  rb_p2p_disconnect_player covers disconnects the user issues;
 * peer-reported disconnects arrive through rb_p2p_receive_peer_connect_status
 * (RB_P2P_FLAG_PEER_STATUS, below).  Spectators are batches of their own
 * (rb_spectator_*, below), fed by rb_p2p_export_confirmed_inputs; registering
 * them on the host (PlayerType::Spectator) is out of scope.  Time sync
 * (frames_ahead, WaitRecommendation, the NetworkStats this path owns) is
 * rb_p2p_time_sync_enable, below.
 * ======================================================================== */
typedef struct rb_p2p rb_p2p;

typedef struct rb_p2p_config {
  int32_t abi_version;    /* = RB_ABI_VERSION */
  int32_t game;           /* rb_game: RB_GAME_EX_GAME, RB_GAME_STUB, RB_GAME_STUB_ENUM, RB_GAME_BRAWLER */
  int32_t num_sessions;
  int32_t num_players;    /* with_num_players (builder.rs:154-157) */
  int32_t max_prediction; /* with_max_prediction_window (builder.rs:136-145) */
  int32_t input_delay;    /* with_input_delay (builder.rs:148-151): local handles */
  int32_t device;
  uint32_t local_mask;    /* bit h: handle h is PlayerType::Local; at least one local and one remote */
  int32_t remote_delay;   /* frame of each remote handle's first Event::Input (the peer's input delay) */
  int32_t sparse_saving;  /* with_sparse_saving_mode (builder.rs:159-166) */
  uint32_t flags;         /* RB_FLAG_LANE_PER_SESSION, RB_P2P_FLAG_FANOUT, RB_P2P_FLAG_PEER_STATUS */
  uint32_t block_size;
  int32_t desync_interval; /* with_desync_detection_mode (builder.rs:167-172): DesyncDetection::On{interval}
                              for interval > 0, Off for 0 (the default, builder.rs:15) */
  int32_t fanout_candidates; /* RB_P2P_FLAG_FANOUT: branches per session, 1..16 (default 16) */
  uint32_t fanout_min_select_permille; /* adaptive fan-out (RB_P2P_FLAG_FANOUT without _ALWAYS): the
                              select fraction of rollbacks below which the batch turns it off;
                              0 = the default, 150 */
  uint32_t reserved[1];
} rb_p2p_config;

/* Speculative branch fan-out (BASELINE config 4): after every tick each session
 * presimulates K = fanout_candidates branches (at most 16), one per candidate
 * input of the remote handle with the oldest unconfirmed input, over its
 * unconfirmed frames.  The candidates are the game's whole input alphabet when
 * it has at most K values (ex_game's 4 input bits, K = 16), else the K most
 * likely values: the most recently confirmed distinct inputs of that handle,
 * newest first (the reference's repeat-last prediction, input_queue.rs:126-140,
 * is candidate 0), then the smallest values not taken.  A later misprediction
 * of that handle alone, held at one candidate value, becomes a branch select
 * instead of LoadGameState + resimulation; cells, states, statuses and frames
 * stay identical to the plain rollback.  Candidates that act alike on the
 * player share one branch (ex_game's 16 inputs are 9 trajectories).  ex_game
 * (one lane per player: the fan-out runs inside the P2P tick, so a call of many
 * ticks is one launch) and the brawler (one wave per session: a fan-out launch
 * between one-tick P2P launches); not with sparse saving. */
#define RB_P2P_FLAG_FANOUT 4u

/* The fan-out is adaptive by default: a batch measures, over windows of 64
 * ticks, the fraction of its rollbacks that became selects; below
 * fanout_min_select_permille it stops presimulating for the next 960 ticks (its
 * ticks run as plain P2P ticks), then measures again.  Presimulation only pays
 * through selects: a stream whose held inputs rarely match a candidate (the
 * brawler's 256-value inputs: 3.8% of rollbacks at 20x the plain tick's cost)
 * gets plain rollback.  The measurement is asynchronous (a device reduction into
 * pinned memory, read when it has landed): no call waits for it.  Results are
 * the same either way.  RB_P2P_FLAG_FANOUT_ALWAYS keeps it on. */
#define RB_P2P_FLAG_FANOUT_ALWAYS 16u

/* Per-player speculation (with RB_P2P_FLAG_FANOUT; games whose players move
 * independently and whose whole input alphabet fits the candidates: ex_game at
 * K = 16): every remote player's input classes are presimulated, each in its
 * own lane, from the oldest first unconfirmed frame B over the remote players,
 * instead of the one remote player with that oldest frame.  A rollback from B
 * in which every remote player's newly confirmed inputs hold one class then
 * becomes a select even when several players mispredicted (the plain fan-out
 * needs the speculated player to be the only one).  More chains per tick: the
 * bench reports both forms (bench.py --fanout-mode). */
#define RB_P2P_FLAG_FANOUT_PER_PLAYER 32u

/* Peers' connect-status reports (update_player_disconnects, p2p_session.rs:707-742):
 * every advance_frame combines what the running endpoints last reported about
 * each player (rb_p2p_receive_peer_connect_status) with the session's own
 * view; a player some peer reports disconnected is disconnected here too, at
 * the earliest reported frame, with the resimulation that implies. */
#define RB_P2P_FLAG_PEER_STATUS 8u

/* SessionBuilder::new() defaults for a 2-player session, handle 0 local, handle 1 remote. */
void rb_p2p_config_init(rb_p2p_config* cfg);

/* The adaptive fan-out's state: *active (1: presimulating), the select fraction of
 * rollbacks of the last measured window (-1: none yet), the windows measured and
 * the times it was turned off.  Does not synchronise.  RB_INVALID_REQUEST without
 * the fan-out. */
rb_status rb_p2p_fanout_state(rb_p2p* b, int32_t* active, double* select_fraction, int32_t* windows,
                              int32_t* turned_off);

/* SessionBuilder::start_p2p_session (builder.rs:251-308) for S sessions that
 * start Running (the synchronisation handshake is the network's). */
rb_status rb_p2p_create(const rb_p2p_config* cfg, rb_p2p** out);
void rb_p2p_destroy(rb_p2p* b);
const char* rb_p2p_last_error(const rb_p2p* b);
rb_status rb_p2p_set_stream(rb_p2p* b, void* hip_stream);
void* rb_p2p_get_stream(const rb_p2p* b);  /* as rb_get_stream */

/* n_ticks x [poll_remote_clients + add_local_input for every local handle +
 * advance_frame (p2p_session.rs:253-337) + handle_requests] for every session,
 * in ONE device launch.  Device pointers, stream ordered:
 *   local_inputs  tick t, handle h: local_inputs + t*local_stride_bytes + (h*S + s)*input_bytes
 *                 (entries of remote handles are ignored)
 *   remote_upto   int32 [n_ticks][num_players][S]: newest frame delivered for
 *                 remote handle h before tick t's advance_frame (monotone;
 *                 entries of local handles ignored)
 *   remote_inputs [remote_frames][num_players][S] Input values by frame (a
 *                 watermark past remote_frames - 1 counts as that), or, after
 *                 rb_p2p_set_delivery_ring(R), the ring [R][num_players][S]
 *                 with remote_frames == R
 * A session that hits PredictionThreshold (sync_layer.rs:163-167) does not
 * advance that tick (rb_p2p_read_status reports it), exactly as the
 * reference's advance_frame returns Err: its bookkeeping moves, its game does
 * not.  Asynchronous (stream ordered): a session that hits a reference assert
 * stops and reports RB_PANIC through rb_p2p_read_status / rb_p2p_counters. */
rb_status rb_p2p_run_ticks(rb_p2p* b, int32_t n_ticks, const void* local_inputs, int64_t local_stride_bytes,
                           const int32_t* remote_upto, const void* remote_inputs, int32_t remote_frames);

/* rb_p2p_run_ticks with the remote inputs arriving as the peers' input packets
 * (the format of rb_encode_input_packets below): each tick first runs
 * UdpProtocol::on_input (protocol.rs:616-689) for every remote endpoint inside
 * the tick's poll_remote_clients, decoding straight into the InputQueue (one
 * launch does decode and tick; the deliveries never pass through
 * remote_upto / remote_inputs).  Device pointers, stream ordered:
 *   packets       tick t, remote handle h, session s: the packet at
 *                 packets + ((t*num_players + h)*S + s)*packet_stride;
 *                 packet_stride a multiple of 16, at least 32; the packet's
 *                 length and start frame at lengths / start_frames[(t*num_players + h)*S + s]
 *                 (length 0: none; entries of local handles ignored)
 *   decode_status NULL, or int32 [num_players][S]: the last tick's result per
 *                 endpoint (the codes of rb_decode_input_packets)
 *   acks          NULL, or int32 [num_players][S]: after the call, the newest
 *                 frame received per endpoint (RB_NULL_FRAME: none), the ack
 *                 the receiver returns to the sender
 * A malformed packet (or a length above packet_stride) panics its session
 * (the reference's decode().expect, "decoding failed", protocol.rs:656); so
 * does a packet that skips frames never received (status -2: the reference's
 * assert!, protocol.rs:639-642).  Sparse saving, the fan-out, desync
 * detection, peers' connect-status reports and max_prediction >= 64 (a
 * reference input up to 2*max_prediction frames back must still be in the
 * 128-entry input ring): RB_INVALID_REQUEST. */
rb_status rb_p2p_run_ticks_packets(rb_p2p* b, int32_t n_ticks, const void* local_inputs, int64_t local_stride_bytes,
                                   const uint8_t* packets, int64_t packet_stride, const int32_t* lengths,
                                   const int32_t* start_frames, int32_t* decode_status, int32_t* acks);

/* P2PSession::disconnect_player(handle) (p2p_session.rs:430-456, 555-581) in
 * every session whose `session_mask` byte is non-zero (NULL: all sessions),
 * called between rb_p2p_run_ticks calls (stream ordered).  Errors as the
 * reference, RB_INVALID_REQUEST with nothing applied: "Invalid Player Handle."
 * (handle >= num_players), "Local Player cannot be disconnected.", "Player
 * already disconnected." (in any selected session).  From then on the player's
 * deliveries are ignored, it leaves the confirmed frame, every frame after its
 * last one advances with (zeroed, Disconnected), and the next advance_frame
 * resimulates from last_frame + 1 if that frame was already simulated. */
rb_status rb_p2p_disconnect_player(rb_p2p* b, int32_t handle, const uint8_t* session_mask);

/* Dropping the P2PSession and calling SessionBuilder::start_p2p_session
 * (builder.rs:251-308) again with the same builder, in every session whose
 * `session_mask` byte is non-zero (host pointer, [S] bytes; NULL: all
 * sessions), called between rb_p2p_run_ticks calls: stream ordered, without a
 * host synchronisation (the mask is consumed before the call returns); an empty
 * selection launches nothing.  Every per-session value of a selected session
 * becomes what rb_p2p_create writes (and rb_p2p_time_sync_enable, the first
 * export and the first paced tick, where the batch has used them): the live
 * state, all cells, the input ring, the bookkeeping rows with their escape and
 * move-to-front rows, the status and trace words (a panicked session runs
 * again), the desync histories, outbox and event ring, the peers'
 * connect-status rows, the export's next_spectator_frame and status
 * (RB_P2P_EXPORT_OVERRUN is cleared), the time-sync rows, windows and
 * WaitRecommendation ring, the pacing view, parked-tick count and accumulator,
 * and the fan-out's branch validity.  A caller that wants a session's events,
 * recommendations or parked count reads them first.  The session's next tick
 * is its frame 0: its deliveries, packets' start frames and export rows count
 * from 0 again.  Unselected sessions are untouched.  Batch-wide values continue
 * since create: rb_p2p_counters, rb_p2p_totals, the adaptive fan-out's policy,
 * the launch clock and the profile events; rb_p2p_time_sync_enable stays
 * closed. */
rb_status rb_p2p_restart_sessions(rb_p2p* b, const uint8_t* session_mask);

/* Moving running sessions between batches.  GGRS has no such call, because a
 * P2PSession is an ordinary movable Rust value; here a session is a column of
 * every per-session buffer of its batch, and a move is an export of the
 * selected columns into session records and an import of records into the
 * selected columns of another batch (or of the same one: a rewind), on another
 * device or in another process if the caller carries the bytes there.
 *
 * A record is a position-independent byte image of one session
 * (ggrs_amd/csrc/session_record.hpp): a 32-byte header
 * (magic, format version, record_bytes, a fingerprint of the batch's plane
 * list and configuration) and every per-session value: all that
 * rb_p2p_restart_sessions resets, and the checksum history, outbox and
 * desync-event payloads behind their counts.  records_dev is device memory,
 * [n][record_bytes] bytes, 16-byte aligned; record k belongs to sessions[k].
 * Records stand on their own: they may be reordered, copied through the host,
 * sent elsewhere or written to disk.  rb_p2p_session_record_bytes depends on
 * the batch's configuration alone (a multiple of 16).
 *
 * `sessions` is a host list of n distinct indices in [0, S), consumed before
 * the call returns; a duplicate or an index out of range is
 * RB_INVALID_REQUEST, refused before any launch; n == 0 is RB_OK without a
 * launch.  Both calls go between rb_p2p_run_ticks calls, are stream ordered on
 * the batch's stream and do not synchronise the host.  Both make the pacing
 * rows and the export's rows if the batch has not used them yet, with create's
 * fresh values (no read-back changes).
 *
 * Export only reads the batch.  Import overwrites the selected sessions'
 * columns and no others.  It checks every record's header on the device
 * against this batch's magic, version, record_bytes and fingerprint: game,
 * num_players, max_prediction, input and state sizes, input and remote delay,
 * local_mask, sparse_saving, desync_interval, RB_P2P_FLAG_PEER_STATUS, time
 * sync on / off and its fps, and the fan-out mode and candidates must agree.
 * A record that does not match leaves its session untouched, in every buffer,
 * and adds 1 to a count rb_p2p_import_refused reads (since create;
 * synchronises).
 *
 * A moved session keeps its own frame numbering: the caller's tensors move
 * with it (the session's columns of remote_inputs, remote_upto, packet start
 * frames, the export rows, its spectators' host_upto).  After an import
 * rb_p2p_time_sync_enable is closed as after a tick, and the next
 * rb_p2p_disconnect_player reads the imported connect status back first.
 * Batch-wide values stay with their batch: rb_p2p_counters, rb_p2p_totals, the
 * adaptive fan-out's policy, the launch clock.  Of a fan-out batch the
 * presimulated branches are not carried: an imported session has no valid
 * branch, as a restarted one, and its next confirmation rolls back; states are
 * identical, only rb_p2p_totals differ. */
int64_t   rb_p2p_session_record_bytes(const rb_p2p* b);
rb_status rb_p2p_export_sessions(rb_p2p* b, const int32_t* sessions, int32_t n, void* records_dev);
rb_status rb_p2p_import_sessions(rb_p2p* b, const int32_t* sessions, int32_t n, const void* records_dev);
rb_status rb_p2p_import_refused(rb_p2p* b, uint32_t* count);   /* read-back: synchronises */

/* Per session, the last tick: rb_status of its advance_frame, the LoadGameState
 * frame (RB_NULL_FRAME: no rollback), AdvanceFrame and SaveGameState counts.
 * Any pointer may be NULL.  Synchronises. */
rb_status rb_p2p_read_status(rb_p2p* b, int32_t* status, int32_t* load_frame, int32_t* n_advance, int32_t* n_save);
/* SyncLayer::current_frame and last_confirmed_frame per session.  Synchronises. */
rb_status rb_p2p_read_frames(rb_p2p* b, int32_t* current, int32_t* confirmed);
/* Every session's InputQueue / ConnectionStatus bookkeeping, out[S][P][RB_P2P_QUEUE_FIELDS]:
 * last_added_frame, inputs[tail].frame, length, last_requested_frame, prediction.frame,
 * first_incorrect_frame (input_queue.rs:12-34), ConnectionStatus::last_frame and
 * disconnected (messages.rs:5-18).  For parity tests and debugging.  Synchronises. */
#define RB_P2P_QUEUE_FIELDS 8
rb_status rb_p2p_read_queues(rb_p2p* b, int32_t* out);
/* All cells: frame tags [W][S], images [W][S][rb_p2p_state_bytes], checksums [W][S][2]. */
rb_status rb_p2p_read_cells(rb_p2p* b, int32_t* tags, void* images, uint64_t* checksums);
/* The game state after the last advance, images [S][rb_p2p_state_bytes] (frame word = current frame). */
rb_status rb_p2p_read_live(rb_p2p* b, void* images);
int32_t rb_p2p_state_bytes(const rb_p2p* b);
int32_t rb_p2p_input_bytes(const rb_p2p* b);
/* Counters since create: [0] PredictionThreshold hits, [1] unexpected math paths, [2] panicked sessions. */
rb_status rb_p2p_counters(rb_p2p* b, uint32_t* out3);
/* Work the device executed since create: [0] AdvanceFrame, [1] SaveGameState,
 * [2] LoadGameState (requests dropped with a PredictionThreshold error
 * excluded), [3] rollbacks replaced by a speculative select, [4] branch frames
 * presimulated by the fan-out. */
rb_status rb_p2p_totals(rb_p2p* b, uint64_t* out5);
/* ---- Desync detection (p2p_session.rs:873-928, protocol.rs:27, 710-742) with
 * desync_interval > 0.  In every advance_frame at current % interval == 0 a
 * session records ChecksumReport{checksum, frame = last_saved_frame - 1} of its
 * cell (only when that frame > max_prediction; no such cell is a reference
 * panic -> RB_PANIC), keeps it in its local checksum history (the newest 32
 * frames), and compares the history each remote endpoint received with it:
 * every differing frame is a GGRSEvent::DesyncDetected{frame, local_checksum,
 * remote_checksum, addr}.  The reports travel between peers through the caller
 * (on one node: an all-gather, ggrs_amd/shard.py), like the datagrams
 * UdpProtocol::send_checksum_report sends. */
#define RB_P2P_REPORTS_PER_TAKE 8 /* reports kept per session between two takes (older ones are dropped, like lost datagrams) */
#define RB_P2P_EVENTS_KEPT 16     /* newest DesyncDetected events kept per session */

/* The reports every session sent since the last call, oldest first, into
 * device memory dev_out[RB_P2P_REPORTS_PER_TAKE][S] rb_checksum_report
 * (frame RB_NULL_FRAME: none; mismatch_frame unused, RB_NULL_FRAME).
 * Stream-ordered. */
rb_status rb_p2p_take_checksum_reports(rb_p2p* b, void* dev_out);

/* UdpProtocol::on_checksum_report (protocol.rs:710-722) for the endpoint of
 * remote handle `handle` of every session: dev_in[k * S + s], k < count,
 * rb_checksum_report in the layout rb_p2p_take_checksum_reports writes (the
 * peer's reports for this session), applied in order.  Stream-ordered.
 * RB_INVALID_REQUEST: handle is not a remote handle, or desync detection is off. */
rb_status rb_p2p_receive_checksum_reports(rb_p2p* b, int32_t handle, const void* dev_in, int32_t count);

/* DesyncDetected events per session: counts[S] since create, and the newest
 * RB_P2P_EVENTS_KEPT in order as frames / remote handles (the `addr`) / local /
 * remote checksum low words, each [S][RB_P2P_EVENTS_KEPT] (frame RB_NULL_FRAME,
 * handle -1: none).  Any pointer may be NULL.  Synchronises. */
rb_status rb_p2p_read_desync_events(rb_p2p* b, uint32_t* counts, int32_t* frames, int32_t* handles,
                                    uint64_t* local_checksums, uint64_t* remote_checksums);

/* UdpProtocol::on_input's merge of the peer's connect status (protocol.rs:627-636)
 * for the endpoint of remote handle `endpoint` in every session: the peer
 * reports player i as last_frames[i * S + s] / disconnected[i * S + s] (device
 * memory, [num_players][S] int32 and uint8); the stored status becomes
 * (stored.disconnected || reported, max(stored.last_frame, reported)).
 * Stream-ordered, between ticks.  RB_INVALID_REQUEST without
 * RB_P2P_FLAG_PEER_STATUS or for a local handle. */
rb_status rb_p2p_receive_peer_connect_status(rb_p2p* b, int32_t endpoint, const int32_t* last_frames,
                                             const uint8_t* disconnected);

/* P2PSession::send_confirmed_inputs_to_spectators (p2p_session.rs:303, 676-703)
 * over SyncLayer::confirmed_inputs (sync_layer.rs:203-217), batched: the feed of
 * a spectator batch (rb_spectator_run_ticks).  Device pointers, stream ordered,
 * called between rb_p2p_run_ticks calls.  Per session, with confirmed = the
 * minimum of ConnectionStatus::last_frame over the players that are not
 * disconnected (confirmed_frame, p2p_session.rs:487-498; not the SyncLayer's
 * clamped last_confirmed_frame): while next_spectator_frame <= confirmed and
 * next_spectator_frame < frames, every player's input of that frame goes to
 *   inputs_by_frame [frames][num_players][S] Input values (the layout and
 *                   absolute frames of rb_p2p_run_ticks's remote_inputs):
 *                   zero for a player with disconnected && last_frame < frame,
 *                   else the InputQueue's entry of the frame
 * and next_spectator_frame (per session, 0 at first: p2p_session.rs:201) moves
 * on.  Then
 *   upto            int32 [S]: the newest frame exported so far (RB_NULL_FRAME: none)
 *   last_frames     int32 [num_players][S], disconnected uint8 [num_players][S]:
 *                   the host's local_connect_status, the peer_connect_status
 *                   its Input messages carry (rb_spectator_receive_host_status)
 * Nothing is written past upto.  Panicked sessions export nothing.
 *
 * The reference sends after every tick, so it never reads an InputQueue slot
 * that a later frame has overwritten.  Here a caller may export rarely: a
 * session in which any queue has added a frame >= next_spectator_frame + 128
 * (the ring holds 128 frames) has lost inputs it still had to send; it exports
 * nothing more, from that call on, and reports RB_P2P_EXPORT_OVERRUN through
 * rb_p2p_read_export_status.  That status is a word of its own: the sticky
 * panic word, rb_p2p_read_status and the session's ticks are untouched.
 *
 * Called after every tick the export equals the reference's per-tick sending.
 * After longer launches it equals it too, except with RB_P2P_FLAG_PEER_STATUS
 * when a peer-reported disconnect lands inside a launch: frames between the
 * player's last frame and the tick it was disconnected in, which the
 * reference had already sent with the player's inputs, are exported zeroed. */
#define RB_P2P_EXPORT_OK 0
#define RB_P2P_EXPORT_OVERRUN 1
rb_status rb_p2p_export_confirmed_inputs(rb_p2p* b, void* inputs_by_frame, int32_t frames, int32_t* upto,
                                         int32_t* last_frames, uint8_t* disconnected);
/* ---- Per-session delivery rings.  By default every
 * by-frame tensor of a batch is linear: [frames][num_players][S], indexed by
 * each session's absolute frame, so it must reach the frame of the batch's
 * oldest session.  Once sessions restart (rb_p2p_restart_sessions) or arrive
 * (rb_p2p_import_sessions) at different times no window of absolute frames
 * serves them all.  A delivered frame is read exactly once, though:
 * Event::Input hands it to the InputQueue (p2p_session.rs:838-852,
 * input_queue.rs:149-204) while ConnectionStatus::last_frame < frame <=
 * remote_upto, and from then on it lives in the batch's own 128-entry ring.
 *
 * rb_p2p_set_delivery_ring(b, R) makes every by-frame tensor argument of the
 * batch a ring of R frames indexed by each session's OWN frame: [R][num_players][S],
 * frame f of session s in slot f & (R - 1).  That is remote_inputs of
 * rb_p2p_run_ticks and rb_p2p_run_ticks_paced and inputs_by_frame of
 * rb_p2p_export_confirmed_inputs and rb_p2p_export_local_inputs.  The matching
 * remote_frames / frames argument must equal R, else RB_INVALID_REQUEST (a
 * linear tensor passed by mistake).  R == 0 returns the batch to the linear
 * layout (the default); otherwise R is a power of two of at least
 * RB_INPUT_QUEUE_LENGTH; anything else is RB_INVALID_REQUEST with nothing
 * changed.  Called between tick calls; host state only: no device state, no
 * synchronisation, session records and their fingerprints are unchanged.
 * rb_p2p_run_ticks_packets has no by-frame tensor and ignores it.  A plug-in
 * game built before the frame mask (no rb_plugin_delivery_ring, plugin.hip)
 * is refused a ring, RB_INVALID_REQUEST; its linear layout runs as before.
 *
 * In ring mode no frame is clamped to the tensor's length: time sync's
 * last_recv (protocol.rs:268-277) and the parked poll's are remote_upto itself.
 *
 * The caller's contract:
 *   - at launch, every frame in (newest frame delivered before the call,
 *     largest watermark of the call] is in its slot, per endpoint;
 *   - that span is at most R frames per endpoint (a poll that adds 128 or more
 *     frames to a non-empty queue fires input_queue.rs:181's assert anyway);
 *   - a slot's earlier content, including a previous match's inputs in a
 *     restarted session's column, is never read: a consumed frame is not read
 *     again, and frames past the watermark are loaded ahead and discarded.
 * Addresses stay inside the tensor whatever the watermarks are; a caller that
 * breaks the contract gets the inputs its slots held, not a fault, and is not
 * detected.
 *
 * rb_p2p_export_confirmed_inputs in ring mode writes frame `next` to slot
 * next & (R - 1) and exports at most R frames per session in one call (no slot
 * twice); the rest follows in the next call, `upto` says where it stopped.  The
 * 128-frame overrun rule and RB_P2P_EXPORT_OVERRUN are unchanged. */
rb_status rb_p2p_set_delivery_ring(rb_p2p* b, int32_t ring_frames);

/* UdpProtocol::send_input (protocol.rs:439-466) as add_local_input calls it for
 * every remote endpoint (p2p_session.rs:330-353), in tensor form: the feed of
 * a peer batch, the twin of rb_p2p_export_confirmed_inputs.  Device pointers,
 * stream ordered, called between tick calls.  For every session and every
 * LOCAL handle h, the inputs of frames sent[h][s] + 1 ..
 * local_connect_status[h].last_frame (the newest frame add_local_input queued:
 * current frame - 1 + input_delay) go from the batch's InputQueue to
 *   inputs_by_frame [frames][num_players][S] Input values, in the batch's
 *                   current layout: linear (frames below `frames` only), or the
 *                   delivery ring (frames == R, frame f in slot f & (R - 1))
 * and then
 *   sent            int32 [num_players][S] = the last frame written.
 * Rows of remote handles, in inputs_by_frame and in sent, are untouched.  sent
 * is the caller's state (pending_output's front, protocol.rs:462-466):
 * RB_NULL_FRAME at first, and again once the caller restarts the session; the
 * library keeps no plane for it.  The frames below input_delay are the blank
 * inputs of the queue's delay fill (input_queue.rs:227-231), which the peer
 * skips (rb_p2p_config.remote_delay).
 * The InputQueue holds the newest 128 frames: a call never goes back further
 * than last_frame - 127; it skips ahead, and the older frames are lost (call
 * at least every 128 ticks).  Panicked sessions export nothing.  Inputs of 1
 * and 4 bytes; else RB_INVALID_REQUEST.
 *
 * Two batches that are each other's peers can share one [R][P][S] ring and one
 * sent tensor: each writes the rows of its own handles and reads the other's,
 * and the caller models latency by handing each side an older copy of sent as
 * its remote_upto. */
rb_status rb_p2p_export_local_inputs(rb_p2p* b, void* inputs_by_frame, int32_t frames, int32_t* sent);

/* Per session: RB_P2P_EXPORT_OK / RB_P2P_EXPORT_OVERRUN and next_spectator_frame
 * (both as the last export left them; before the first: OK and 0).  Either
 * pointer may be NULL.  Synchronises. */
rb_status rb_p2p_read_export_status(rb_p2p* b, int32_t* status, int32_t* next_frame);

/* ---- Time sync (time_sync.rs; protocol.rs:268-277, 439-455, 697-708;
 * p2p_session.rs:745-776).  Every endpoint keeps two 30-frame windows of its
 * local and remote frame advantage; a session's frames_ahead is the maximum
 * over its connected remote players of the windows' halved average difference,
 * and every 60 frames at most a session that runs 3 or more frames ahead
 * raises GGRSEvent::WaitRecommendation{skip_frames} (lib.rs:151-155).  Time
 * sync never feeds back into a session inside a call: it runs as a launch of
 * its own after the ticks of every rb_p2p_run_ticks call, on the batch's
 * stream, from a per-tick log those ticks write, and
 * the caller acts on its results between calls.
 *
 * rb_p2p_time_sync_enable is SessionBuilder::with_fps (builder.rs:186-199):
 * fps <= 0 is RB_INVALID_REQUEST "FPS should be higher than 0."; so is a second
 * call, or a call after the batch's first tick.  rb_p2p_config is unchanged.
 * Works with every configuration of rb_p2p_run_ticks (sparse saving, desync
 * detection, peers' connect status, both fan-out forms);
 * rb_p2p_run_ticks_packets with time sync on is RB_INVALID_REQUEST (there the
 * newest received frame is decided inside the kernel).  Per tick, with cur =
 * current_frame at the tick's entry: every remote handle h still connected at
 * the tick's entry takes last_recv = min(remote_upto[t][h][s], remote_frames - 1)
 * and, unless that is RB_NULL_FRAME, local_frame_advantage[h] = last_recv +
 * ((rtt_ms[h] / 2) * fps) / 1000 - cur (i32, truncating); frames_ahead and the
 * event follow; a tick that gets past add_local_input (no
 * PredictionThreshold) writes both windows at slot (cur + input_delay) % 30 for
 * every remote handle connected after update_player_disconnects.  A session
 * that panics stops its time sync at that tick.
 * The tick log grows to the largest n_ticks a call has passed: a call with more
 * ticks than any before it (the first included) synchronises the batch's
 * stream and allocates inside rb_p2p_run_ticks.  A caller that captures its
 * launches into a graph makes one uncaptured call of its largest n_ticks first. */
#define RB_P2P_WAIT_EVENTS_KEPT 8 /* newest WaitRecommendation events kept per session */
rb_status rb_p2p_time_sync_enable(rb_p2p* b, int32_t fps);

/* UdpProtocol::on_quality_reply / on_quality_report (protocol.rs:697-708) for
 * the endpoint of remote handle `handle` in every session: round_trip_time in
 * milliseconds and the peer's frame advantage, device int32 [S] each; either
 * may be NULL, which leaves that value as it is.  Stream ordered, called between
 * rb_p2p_run_ticks calls.  frame_advantage is an i8 on the wire: the caller
 * keeps it in -128..127; rtt_ms must keep (rtt_ms / 2) * fps inside int32.
 * RB_INVALID_REQUEST: a local handle, or time sync off. */
rb_status rb_p2p_receive_quality(rb_p2p* b, int32_t handle, const int32_t* rtt_ms, const int32_t* frame_advantage);

/* frames_ahead (p2p_session.rs:551) into frames_ahead_dev int32 [S] and every
 * endpoint's local_frame_advantage, the payload of the QualityReport the batch
 * owes its peer (protocol.rs:516-524), into local_adv_dev int32 [num_players][S]
 * (0 for local handles): device memory, stream ordered, no synchronisation.
 * Either pointer may be NULL. */
rb_status rb_p2p_export_time_sync(rb_p2p* b, int32_t* frames_ahead_dev, int32_t* local_adv_dev);

/* The same to host arrays, with the rest of NetworkStats this path owns
 * (protocol.rs:294-300): frames_ahead [S]; local_adv (local_frames_behind),
 * remote_adv (remote_frames_behind) and rtt_ms (ping), each [num_players][S].
 * send_queue_len and kbps_sent are the network layer's.  Any pointer may be
 * NULL.  Synchronises. */
rb_status rb_p2p_read_time_sync(rb_p2p* b, int32_t* frames_ahead, int32_t* local_adv, int32_t* remote_adv,
                                int32_t* rtt_ms);

/* WaitRecommendation events per session: counts[S] since enable, and the newest
 * RB_P2P_WAIT_EVENTS_KEPT in order as current_frame / skip_frames, each
 * [S][RB_P2P_WAIT_EVENTS_KEPT] (frame RB_NULL_FRAME, skip_frames 0: none).  Any
 * pointer may be NULL.  Synchronises. */
rb_status rb_p2p_read_wait_recommendations(rb_p2p* b, uint32_t* counts, int32_t* frames, int32_t* skip_frames);

/* For tests: the windows, out[2 local, remote][30][num_players][S].  Synchronises. */
rb_status rb_p2p_debug_read_time_sync_windows(rb_p2p* b, int32_t* out);

/* ---- Per-session pacing: the caller's frame loop of
 * examples/ex_game/ex_game_p2p.rs:80-122, where poll_remote_clients runs on
 * every iteration (:84), add_local_input and advance_frame only when the
 * session's own accumulator says a frame is due (:107-122), and a session that
 * is ahead stretches its frame time by 10% (:91-104).
 *
 * rb_p2p_run_ticks_paced is rb_p2p_run_ticks with a run mask: device uint8
 * [n_ticks][S], 0 = parked.  A tick in which session s is parked runs
 * poll_remote_clients for s (the deliveries of remote_upto / remote_inputs enter
 * its input queues and connect status; with time sync on,
 * update_local_frame_advantage of its running endpoints, protocol.rs:268-277)
 * and nothing else: no add_local_input (its local inputs of that tick are
 * ignored), no advance_frame, no request.  Its state, cells, frames, the
 * status and request counts rb_p2p_read_status reports (those of its last
 * advance_frame), its share of rb_p2p_totals, frames_ahead and the time-sync
 * windows stay as they were.  input_queue.rs:181's assert fired by a parked
 * poll (a session parked while deliveries go on for more than 128 frames)
 * panics the session like a running tick's poll.  Running sessions do exactly
 * what rb_p2p_run_ticks does.  run_mask == NULL is rb_p2p_run_ticks itself.
 * A call of n_ticks is n_ticks one-tick sequences on the stream (pacing is for
 * live play, one tick per call), each two small launches more than an unpaced
 * one-tick call.  Sparse saving, desync detection, peers' connect-status
 * reports, disconnects and time sync on or off all work.  RB_INVALID_REQUEST
 * with nothing applied: a batch with the fan-out.  Packet-fed ticks have no
 * paced form. */
rb_status rb_p2p_run_ticks_paced(rb_p2p* b, int32_t n_ticks, const void* local_inputs, int64_t local_stride_bytes,
                                 const int32_t* remote_upto, const void* remote_inputs, int32_t remote_frames,
                                 const uint8_t* run_mask);

/* The pacer: frames_ahead of every session into the next tick's run mask,
 * run_mask_dev device uint8 [S], stream ordered, no host round trip.  The
 * integer form of ex_game_p2p.rs:91-104 for a batch ticking at the nominal
 * frame rate, with a per-session accumulator that starts at 0:
 *   acc += 10; cost = frames_ahead > 0 ? 11 : 10; run = acc >= cost; if (run) acc -= cost;
 * so a session never ahead runs every tick and a session held ahead runs 10 of
 * every 11.  A panicked session gets 1.  RB_INVALID_REQUEST: time sync off. */
rb_status rb_p2p_pace(rb_p2p* b, uint8_t* run_mask_dev);

/* Ticks each session was parked in since create, parked_ticks [S] (counted by
 * the paced ticks, whatever made their masks).  Synchronises. */
rb_status rb_p2p_read_pacing(rb_p2p* b, uint32_t* parked_ticks);

/* ---- Endpoint liveness: deciding that a peer has gone
 * silent.  UdpProtocol keeps last_recv_time and two flags per endpoint:
 * handle_message stamps the time on every message of any kind and raises
 * NetworkResumed if the notify had been sent (network/protocol.rs:555-562);
 * on_input raises Disconnected when the peer's Input carries
 * disconnect_requested (:621-626); poll raises NetworkInterrupted after
 * disconnect_notify_start without a message and Disconnected after
 * disconnect_timeout (:377-394).  P2PSession::handle_event forwards the first
 * two and answers Disconnected with disconnect_player_at_frame(handle,
 * local_connect_status[handle].last_frame) (sessions/p2p_session.rs:818-847).
 * The sockets stay the caller's; the timers need only its clock and one
 * "something arrived" byte per endpoint.  An optional group of a P2P batch:
 * off unless enabled, and with it off nothing changes anywhere.
 *
 * rb_p2p_liveness_enable is SessionBuilder::with_disconnect_timeout /
 * with_disconnect_notify_delay (builder.rs:175-184; the defaults are 2000 and
 * 500 ms).  RB_INVALID_REQUEST with nothing changed: a second call; delays
 * outside 0 <= notify_start_ms <= disconnect_timeout_ms (the Duration
 * subtraction of protocol.rs:381 panics where the notify delay exceeds the
 * timeout).  Before or after the first tick: no tick kernel reads its planes.
 * Works with every configuration of rb_p2p_run_ticks, rb_p2p_run_ticks_paced
 * (a parked session is polled like any other) and rb_p2p_run_ticks_packets.
 * rb_p2p_restart_sessions resets the selected sessions' stamps, flags and
 * event count; a move carries them, between batches with equal delays only
 * (they enter the fingerprint when liveness is on; a batch without it keeps
 * the record and fingerprint it had).  The stamps are the caller's clock: two
 * batches that exchange records share one clock. */
#define RB_P2P_NET_EVENTS_KEPT 16 /* newest network events kept per session */
#define RB_NET_INTERRUPTED 1   /* value = disconnect_timeout_ms - notify_start_ms (protocol.rs:381-384) */
#define RB_NET_RESUMED 2       /* protocol.rs:559-562 */
#define RB_NET_DISCONNECTED 3  /* protocol.rs:388-394, 621-626 */
rb_status rb_p2p_liveness_enable(rb_p2p* b, int32_t disconnect_timeout_ms, int32_t notify_start_ms);

/* The timer half of one poll_remote_clients (p2p_session.rs:375-415) for every
 * session: one launch, stream ordered, no synchronisation.  Called between
 * tick calls, before the tick call whose watermarks deliver what this poll
 * received.  now_ms: the caller's clock in milliseconds, >= 0 and never below
 * the previous call's (else RB_INVALID_REQUEST, nothing launched).  Device
 * uint8 [num_players][S] each, entries of local handles ignored / written 0:
 *   received              non-zero: at least one message of any kind came from
 *                         that endpoint since the previous poll
 *   disconnect_requested  may be NULL; the flag of the peer's Input message
 *   state_out             may be NULL; the flags after the call: bit 0
 *                         disconnect_notify_sent, bit 1 disconnect_event_sent,
 *                         bit 2 the player is disconnected
 * A panicked session is skipped.  Otherwise every remote handle is taken in
 * ascending order; a handle whose ConnectionStatus::disconnected is set still
 * stamps but raises nothing (its endpoint no longer runs, protocol.rs:396-401).
 * For the others, in this order:
 *   1. an endpoint that has met no poll yet is stamped now_ms (the reference
 *      stamps at construction, :260: a deviation of at most one poll);
 *   2. received: the stamp becomes now_ms; bit 0 set: cleared, RB_NET_RESUMED;
 *   3. disconnect_requested and bit 1 clear: bit 1 set, RB_NET_DISCONNECTED;
 *   4. bit 0 clear and stamp + notify_start_ms < now_ms: bit 0 set,
 *      RB_NET_INTERRUPTED with value disconnect_timeout_ms - notify_start_ms;
 *   5. bit 1 clear and stamp + disconnect_timeout_ms < now_ms: bit 1 set,
 *      RB_NET_DISCONNECTED;
 *   6. a RB_NET_DISCONNECTED of this poll disconnects the player exactly as
 *      rb_p2p_disconnect_player does (resimulation from last_frame + 1).
 * Both comparisons are strict, in 64 bits.  A session's events of one poll are
 * ordered by handle, then as above (the reference walks a HashMap of
 * endpoints: it has no order across handles).  The next
 * rb_p2p_disconnect_player reads the connect status back first, so "Player
 * already disconnected." holds for a player the timers disconnected. */
rb_status rb_p2p_poll_liveness(rb_p2p* b, int64_t now_ms, const uint8_t* received,
                               const uint8_t* disconnect_requested, uint8_t* state_out);

/* Network events per session: counts[S] since enable or restart, and the newest
 * RB_P2P_NET_EVENTS_KEPT in order as kinds (RB_NET_*) / remote handles / values,
 * each [S][RB_P2P_NET_EVENTS_KEPT] (kind 0, handle -1, value 0: none).  Any
 * pointer may be NULL.  Synchronises. */
rb_status rb_p2p_read_network_events(rb_p2p* b, uint32_t* counts, int32_t* kinds, int32_t* handles, int32_t* values);

/* last_recv_time in the caller's milliseconds (-1: no poll yet, and local
 * handles) as last_recv_ms int64 [num_players][S], and rb_p2p_poll_liveness's
 * state_out bits as state uint8 [num_players][S].  Either may be NULL.
 * Synchronises. */
rb_status rb_p2p_read_liveness(rb_p2p* b, int64_t* last_recv_ms, uint8_t* state);

/* TimeSync::average_frame_advantage (time_sync.rs:30-39) from the windows' sums
 * for n host (local_sum, remote_sum) pairs: device < 0 on the host, else by a
 * kernel on that device (the same function, time_sync.hpp). */
rb_status rb_debug_time_sync_average(int32_t device, const int32_t* local_sums, const int32_t* remote_sums,
                                     int32_t* out, int64_t n);

/* Fault injection for tests (ex_game.rs:211-215 trigger_desync, generalised):
 * XOR `xor_mask` into canonical state word `word` of `session`'s live state
 * and of every cell it holds (checksums unchanged), between ticks. */
rb_status rb_p2p_debug_corrupt(rb_p2p* b, int32_t session, int32_t word, uint32_t xor_mask);

/* HIP event timing of every rb_p2p_run_ticks launch (bench.py): total ms and launches since the last take. */
rb_status rb_p2p_profile_enable(rb_p2p* b, int32_t on);
rb_status rb_p2p_profile_take(rb_p2p* b, double* total_ms, int32_t* launches);
/* rb_launch_clock_arm / _read for P2P batches: every p2p_kernel launch, and
 * with the two-launch fan-out every fanout_kernel launch, takes a slot. */
rb_status rb_p2p_launch_clock_arm(rb_p2p* b, int32_t launches);
rb_status rb_p2p_launch_clock_read(rb_p2p* b, uint64_t* start_end, int32_t cap, int32_t* launches);

/* ===========================================================================
 * SpectatorSession batches (sessions/p2p_spectator_session.rs) — rollback-free
 * replicas of host sessions.
 *
 * S independent spectators, each following one host session: a spectator
 * advances only on inputs the host has confirmed and sent
 * (rb_p2p_export_confirmed_inputs), one frame per tick, or catchup_speed
 * frames while it is more than max_frames_behind frames behind
 * (p2p_spectator_session.rs:109-139).  As for the P2P batches the network
 * layer is the caller's: per tick it passes the newest frame the host's Input
 * messages have delivered and the inputs by frame; the host's connect status
 * goes through rb_spectator_receive_host_status.  Time sync,
 * WaitRecommendation, NetworkStats and the handshake are out of scope: the
 * sessions start Running.
 *
 * A spectator's state after frame c is bit-identical to the cell the host
 * saved for frame c + 1 once that frame is confirmed, and rb_spectator_read_live
 * returns it with that cell's checksum.
 * ======================================================================== */
typedef struct rb_spectator rb_spectator;

typedef struct rb_spectator_config {
  int32_t abi_version;       /* = RB_ABI_VERSION */
  int32_t game;              /* rb_game, as rb_p2p_config.game */
  int32_t num_sessions;
  int32_t num_players;       /* with_num_players (builder.rs:154-157): the host's */
  int32_t device;
  int32_t max_frames_behind; /* with_max_frames_behind (builder.rs:210-225), default 10 */
  int32_t catchup_speed;     /* with_catchup_speed (builder.rs:229-244), default 1 */
  uint32_t block_size;
  uint32_t reserved[4];
} rb_spectator_config;

/* SessionBuilder::new() defaults (builder.rs:13, 23-25): 2 players, 10 frames behind, catch-up speed 1. */
void rb_spectator_config_init(rb_spectator_config* cfg);

/* SessionBuilder::start_spectator_session (builder.rs:310-334) for S sessions
 * that start Running.  Validated before any device work, on the final values,
 * RB_INVALID_REQUEST with the reference's messages (rb_spectator_last_error(NULL)):
 * "Max frames behind cannot be smaller than 1.", "Max frames behind cannot be
 * larger or equal than the Spectator buffer size (60)", "Catchup speed cannot
 * be smaller than 1.", "Catchup speed cannot be larger or equal than the
 * allowed maximum frames behind host"; then the game and player-count rules
 * of rb_p2p_create. */
rb_status rb_spectator_create(const rb_spectator_config* cfg, rb_spectator** out);
void rb_spectator_destroy(rb_spectator* b);
const char* rb_spectator_last_error(const rb_spectator* b);
rb_status rb_spectator_set_stream(rb_spectator* b, void* hip_stream);
void* rb_spectator_get_stream(const rb_spectator* b); /* as rb_get_stream */

/* The host's connect status as its Input messages carry it (handle_event's
 * Event::Input, p2p_spectator_session.rs:243-245, over UdpProtocol::on_input's
 * merge, protocol.rs:629-636): last_frames int32 [num_players][S] and
 * disconnected uint8 [num_players][S], device memory (what
 * rb_p2p_export_confirmed_inputs writes); the stored status becomes
 * (stored.disconnected || reported, max(stored.last_frame, reported)).
 * Stream ordered before the next launch. */
rb_status rb_spectator_receive_host_status(rb_spectator* b, const int32_t* last_frames, const uint8_t* disconnected);

/* start_spectator_session again for every session whose `session_mask` byte
 * is non-zero (rb_p2p_restart_sessions' convention; NULL: all), between
 * rb_spectator_run_ticks calls, stream ordered: the state, checksum, frames,
 * last status and host connect status become what rb_spectator_create writes,
 * so the spectator follows its host's next match from frame 0.  Unselected
 * sessions are untouched; rb_spectator_totals continues since create. */
rb_status rb_spectator_restart_sessions(rb_spectator* b, const uint8_t* session_mask);

/* rb_p2p_export_sessions / rb_p2p_import_sessions for spectators: a spectator
 * moves with its host by the same calls on its own batch.  Its record holds
 * the live state and checksum, current and last received frame, the last
 * status and the host connect status; the fingerprint covers game,
 * num_players, the input and state sizes, max_frames_behind and
 * catchup_speed.  rb_spectator_totals stays with the batch. */
int64_t   rb_spectator_session_record_bytes(const rb_spectator* b);
rb_status rb_spectator_export_sessions(rb_spectator* b, const int32_t* sessions, int32_t n, void* records_dev);
rb_status rb_spectator_import_sessions(rb_spectator* b, const int32_t* sessions, int32_t n, const void* records_dev);
rb_status rb_spectator_import_refused(rb_spectator* b, uint32_t* count);   /* read-back: synchronises */

/* n_ticks x SpectatorSession::advance_frame (+ handle_requests) for every
 * session, in ONE device launch.  Device pointers, stream ordered:
 *   host_upto   int32 [n_ticks][S]: the newest frame delivered before tick t's
 *               advance_frame (RB_NULL_FRAME: none yet; a value below the
 *               session's last_recv_frame changes nothing; a value >= frames
 *               counts as frames - 1)
 *   host_inputs [frames][num_players][S] Input values by frame, complete up to
 *               the largest host_upto of the call
 * Per tick and session: last_recv_frame = max(last_recv_frame, host_upto); then
 * one frame, or catchup_speed frames when last_recv_frame - current_frame >
 * max_frames_behind.  A session whose next frame has not arrived does not
 * advance (RB_PREDICTION_THRESHOLD); one whose next frame left the 60-frame
 * spectator buffer (last_recv_frame >= frame + 60) never advances again
 * (RB_SPECTATOR_TOO_FAR_BEHIND).  A player the host status reports
 * disconnected before the frame advances as (zeroed, Disconnected).
 * With a delivery ring (rb_spectator_set_delivery_ring) host_inputs is
 * [R][num_players][S], frames == R, host_upto is never clamped, and the ring's
 * head may lead the host_upto handed here by at most R - 60 frames. */
rb_status rb_spectator_run_ticks(rb_spectator* b, int32_t n_ticks, const int32_t* host_upto, const void* host_inputs,
                                 int32_t frames);

/* rb_p2p_set_delivery_ring for a spectator batch: host_inputs becomes a ring
 * [R][num_players][S] indexed by each spectator's own frame (frame f in slot
 * f & (R - 1)), what a host batch in ring mode exports, and `frames` must equal
 * R (else RB_INVALID_REQUEST).  R == 0: linear (the default); otherwise a power
 * of two of at least RB_INPUT_QUEUE_LENGTH; anything else RB_INVALID_REQUEST
 * with nothing changed.  Between tick calls, host state only.  In ring mode
 * last_recv_frame = max(last_recv_frame, host_upto), unclamped.
 * A spectator reads frame f when its current_frame reaches f - 1, and never
 * once last_recv_frame >= f + 60 (inputs_at_frame,
 * p2p_spectator_session.rs:177-187, then answers SpectatorTooFarBehind).  So
 * at launch every frame in (current_frame, largest host_upto of the call] that
 * is younger than host_upto - 60 must still be in its slot: the ring's head
 * (the newest frame the host has exported into it) may lead the host_upto a
 * spectator is handed by at most R - 60 frames.  Older content of a slot is
 * never read. */
rb_status rb_spectator_set_delivery_ring(rb_spectator* b, int32_t ring_frames);

/* Per session, the last tick: its rb_status (RB_OK, RB_PREDICTION_THRESHOLD,
 * RB_SPECTATOR_TOO_FAR_BEHIND) and AdvanceFrame count (-1 before the first
 * tick).  Either pointer may be NULL.  Synchronises. */
rb_status rb_spectator_read_status(rb_spectator* b, int32_t* status, int32_t* n_advance);
/* current_frame and last_recv_frame per session (RB_NULL_FRAME at first,
 * p2p_spectator_session.rs:67-68); frames_behind_host (:80-84) is their difference.  Synchronises. */
rb_status rb_spectator_read_frames(rb_spectator* b, int32_t* current, int32_t* last_recv);
/* The game state after frame current_frame, images [S][rb_spectator_state_bytes]
 * (frame word = current_frame + 1), and checksums [S][2] (lo, hi): the
 * checksum of the host's cell of frame current_frame + 1 (every launch stores
 * it; zero before the first).  Either may be NULL.  Synchronises. */
rb_status rb_spectator_read_live(rb_spectator* b, void* images, uint64_t* checksums);
/* Since create: [0] AdvanceFrames executed, [1] ticks that returned
 * PredictionThreshold, [2] ticks that returned SpectatorTooFarBehind (summed over sessions). */
rb_status rb_spectator_totals(rb_spectator* b, uint64_t* out3);
int32_t rb_spectator_state_bytes(const rb_spectator* b);
int32_t rb_spectator_input_bytes(const rb_spectator* b);

/* ===========================================================================
 * Batched input packets (network/compression.rs): one
 * endpoint per (session, remote handle), one packet per endpoint per call.
 * Wire format: XOR delta of every pending input against the reference input,
 * then bitfield RLE (bitfield-rle 0.2 format).  All pointers are device
 * memory; `stream` is a hipStream_t (NULL: the null stream).
 * ======================================================================== */

/* UdpProtocol::on_input (protocol.rs:616-689) for every session's endpoint of
 * remote handle `handle`: packet s is packets + s*packet_stride, lengths[s]
 * bytes (0: none), covering frames start_frames[s]... .  It is decoded against
 * the input before its start frame (remote_inputs, or the zeroed input before
 * the first one), inputs of frames after remote_upto[handle][s] are written to
 * remote_inputs[frame][num_players][num_sessions] (input_bytes each) and
 * remote_upto advances: exactly the delivery tensors rb_p2p_run_ticks reads.
 * status[s]: 0 new inputs, 1 nothing new, -1 malformed (the reference panics:
 * "decoding failed"; also a length above packet_stride), -2 frames missing
 * before start_frame (the reference asserts).  The caller decides what a
 * negative status does to the session (nothing is decoded for it: the packet
 * is validated as a whole before its first input is written).
 * A packet whose reference input is older than 2*max_prediction frames is
 * ignored (recv_inputs retention, protocol.rs:686-688).  Inputs of frames at or
 * above remote_frames are not written, and remote_upto stops at the last frame
 * written.
 * Segment headers are unsigned LEB128 varints (csrc/wire_varint.hpp, shared with the
 * decoder inside rb_p2p_run_ticks_packets).  Accepted: up to ten bytes whose value is
 * below 2^32, so a header padded with continuation groups of zero payload (0x80 ...
 * 0x00) past its fifth byte decodes like its short form, and payload bits 1-6 of a
 * tenth byte (past bit 63) are dropped.  Malformed: a header cut off by the packet's
 * end or still continued after ten bytes, and any header whose value reaches 2^32
 * (bits 32-34 of the fifth byte, any payload bit of bytes six to nine, bit 0 of the
 * tenth): it is neither a run of at most 65,536 bytes nor a literal that fits. */
rb_status rb_decode_input_packets(int32_t device, void* stream, int32_t handle, int32_t num_players,
                                  int32_t num_sessions, int32_t input_bytes, int32_t max_prediction,
                                  const uint8_t* packets, int64_t packet_stride, const int32_t* lengths,
                                  const int32_t* start_frames, void* remote_inputs, int32_t remote_frames,
                                  int32_t* remote_upto, int32_t* status);

/* UdpProtocol::send_pending_output (protocol.rs:468-500) for every session's
 * endpoint: the inputs of handle `handle` for frames acked[s]+1 .. newest[s]
 * (first_frame .. newest[s] before any ack: the sender's input delay) from
 * inputs[frame][num_players][num_sessions], encoded against the input of frame
 * acked[s] (zeroed when acked[s] = RB_NULL_FRAME).  Writes the packet, its
 * length (0: nothing pending, -1: larger than packet_stride) and start frame. */
rb_status rb_encode_input_packets(int32_t device, void* stream, int32_t handle, int32_t num_players,
                                  int32_t num_sessions, int32_t input_bytes, const void* inputs, int32_t frames,
                                  int32_t first_frame, const int32_t* acked, const int32_t* newest, uint8_t* packets,
                                  int64_t packet_stride, int32_t* lengths, int32_t* start_frames);

/* ---- The codec for every endpoint of a batch in one launch, into and out of
 * a linear tensor or a delivery ring.  Stateless like
 * the pair above.  The endpoint of handle h, session s has its packet at
 * packets + (h*S + s)*packet_stride and its length and start frame at
 * lengths[h*S + s] and start_frames[h*S + s]: one tick of
 * rb_p2p_run_ticks_packets' layout, so one packet tensor feeds either path.
 * upto, status, acked and newest are int32 [num_players][S]; upto is a
 * remote_upto row of rb_p2p_run_ticks (and the ack the receiver returns to
 * the sender), newest the `sent` tensor of rb_p2p_export_local_inputs.
 * handle_mask: the handles served.  Every row of a handle outside it is
 * untouched, in every tensor.
 * packet_stride is a multiple of 16 of at least 32 and packets is 16-byte
 * aligned (the rule of rb_p2p_run_ticks_packets).
 * ring_frames == 0: `inputs` is linear, [frames][num_players][S].
 * ring_frames == R: `inputs` is a delivery ring [R][num_players][S], frame f
 * in slot f & (R - 1); no frame is clamped.
 * RB_INVALID_REQUEST, with nothing launched and no tensor touched: an empty
 * mask or bits at or above num_players; num_players > 4; input_bytes not 1, 2
 * or 4; a bad stride or alignment; ring_frames neither 0 nor a power of two of
 * at least RB_INPUT_QUEUE_LENGTH; ring_frames != 0 with frames != ring_frames
 * (the rule of rb_p2p_set_delivery_ring); in decode, 2*max_prediction >=
 * ring_frames (a packet's reference input may be that old and must still be
 * in the ring).
 * Addresses stay inside the tensors for any lengths, start_frames, upto, acked
 * and newest; results are defined for frames below 2^30.  Frames near
 * INT32_MAX are out of range: nothing faults, the values are unspecified.
 *
 * Decode, linear: per endpoint bit for bit rb_decode_input_packets (status
 * codes, the start - 1 >= frames refusal, no write at or above `frames`,
 * validate-then-write).
 * Decode, ring: the same checks in the same order (nothing / overlong / gap /
 * stale reference / negative reference); the reference input is read from slot
 * (start - 1) & (R - 1) before any store; the whole packet is validated, then
 * written.  At most the first R frames above upto are written (no slot twice)
 * and upto stops at the last frame written, so the sender, acked that far,
 * sends the rest again (as rb_p2p_export_confirmed_inputs does in ring mode).
 * The caller's contract: the consumer (rb_p2p_run_ticks, rb_spectator_run_ticks)
 * has read every frame up to the upto handed in; then the frames written here
 * overwrite only consumed slots, and after the call the contract of
 * rb_p2p_set_delivery_ring holds for the new upto. */
rb_status rb_decode_input_packets_all(int32_t device, void* stream, uint32_t handle_mask, int32_t num_players,
                                      int32_t num_sessions, int32_t input_bytes, int32_t max_prediction,
                                      const uint8_t* packets, int64_t packet_stride, const int32_t* lengths,
                                      const int32_t* start_frames, void* inputs, int32_t frames, int32_t ring_frames,
                                      int32_t* upto, int32_t* status);

/* Encode, linear: lengths, start_frames and the packet's bytes are those of
 * rb_encode_input_packets (bytes of the row past the packet's length are
 * unspecified: the packet's first 32 bytes are stored as 16-byte words).
 * Encode, ring: frames acked + 1 .. newest (first_frame .. newest before any
 * ack) are read from their slots and the reference from slot acked & (R - 1).
 * If frames (acked, or the start frame before any ack) .. newest do not fit R
 * distinct slots the reference input has been overwritten: lengths = -2, no
 * packet is written, start_frames is still set.  (The reference raises
 * Event::Disconnected once more than 128 inputs are pending,
 * protocol.rs:461-463; the caller decides what -2 means.)  0: nothing pending,
 * -1: the packet does not fit packet_stride, as above. */
rb_status rb_encode_input_packets_all(int32_t device, void* stream, uint32_t handle_mask, int32_t num_players,
                                      int32_t num_sessions, int32_t input_bytes, const void* inputs, int32_t frames,
                                      int32_t ring_frames, int32_t first_frame, const int32_t* acked,
                                      const int32_t* newest, uint8_t* packets, int64_t packet_stride, int32_t* lengths,
                                      int32_t* start_frames);

/* ---- The codec for endpoints that carry several handles in one stream
 * (DESIGN.md section 21): a remote peer with more than one local player, and
 * every spectator endpoint.  InputBytes::from_inputs (network/protocol.rs:61-79)
 * concatenates the inputs of the endpoint's handles, ascending, into one byte
 * string per frame; send_pending_output XOR-deltas and RLE-codes that string,
 * and on_input's to_player_inputs (:81-93) splits it again.
 * A group is a non-empty set of handles whose inputs travel so; its lead is its
 * lowest handle.  The endpoint of a group in session s owns row lead*S + s of
 * every [P][S] endpoint tensor (packets, lengths, start_frames, acked, newest,
 * status), so the datagram, protocol and liveness calls serve it under a
 * handle_mask of the leads.  A frame of a group of k handles is k*input_bytes
 * bytes (1 to 16): member 0's input, then member 1's, and so on.
 * group_masks: byte g is the handle mask of group g, 0 for no group; up to four
 * groups in any order.
 * Tensor layouts, the linear and ring modes, stride and alignment rules and
 * stream ordering are those of the _all pair above.  Stateless like it.
 * RB_INVALID_REQUEST, with nothing launched and no tensor touched: whatever the
 * _all pair refuses; all four bytes zero; a bit at or above num_players; two
 * groups sharing a handle.
 * Addresses stay inside the tensors for any lengths, start_frames, upto, acked,
 * newest and packet bytes; results are defined for frames below 2^30.
 *
 * Decode: lengths, start_frames, upto and the packet are read from the lead's
 * row only.  The reference input is the members' inputs of frame start - 1 one
 * after the other (zeroed where _all's is).  The checks and status codes are
 * _all's, in its order (nothing / overlong / gap / stale reference / negative
 * reference / linear range), and one more malformed packet: a stream that is
 * not a whole number of frames of k*input_bytes bytes.  The packet is
 * validated as a whole before the first store; every new frame then writes
 * each member's column (the first R frames above upto, no slot twice).  When the
 * packet was taken (status 0, or 1 because it held nothing new) the new
 * watermark goes to the upto row of every member, so rb_p2p_run_ticks and
 * rb_spectator_run_ticks read what they read today; otherwise no upto row is
 * written.  status is written in the lead's row only.  No other row of any
 * tensor is touched. */
rb_status rb_decode_input_packets_grouped(int32_t device, void* stream, uint32_t group_masks, int32_t num_players,
                                          int32_t num_sessions, int32_t input_bytes, int32_t max_prediction,
                                          const uint8_t* packets, int64_t packet_stride, const int32_t* lengths,
                                          const int32_t* start_frames, void* inputs, int32_t frames, int32_t ring_frames,
                                          int32_t* upto, int32_t* status);

/* Encode: acked and newest are read from the lead's row; frames acked + 1 ..
 * newest (first_frame .. newest before any ack) from every member's column; the
 * packet, its length and start frame go to the lead's row.  0, -1 and -2 mean
 * what they mean in rb_encode_input_packets_all, and the segments are chosen as
 * there: the bytes are the reference's encoding of the concatenated frames.
 * A group of one handle writes, byte for byte, what _all writes for that
 * handle. */
rb_status rb_encode_input_packets_grouped(int32_t device, void* stream, uint32_t group_masks, int32_t num_players,
                                          int32_t num_sessions, int32_t input_bytes, const void* inputs, int32_t frames,
                                          int32_t ring_frames, int32_t first_frame, const int32_t* acked,
                                          const int32_t* newest, uint8_t* packets, int64_t packet_stride,
                                          int32_t* lengths, int32_t* start_frames);

/* ---- GGRS's wire messages for every endpoint of a batch in one launch
 * (DESIGN.md section 19): the datagrams the reference puts on its socket,
 * Message { header: { magic }, body: MessageBody } under bincode::serialize
 * (network/messages.rs, network/udp_socket.rs:31-45).  Stateless like the codec
 * above and laid out like it: the endpoint of handle h, session s is row
 * h*S + s of every [P][S] tensor, handle_mask selects the handles served, and
 * no row of a handle outside it is touched, in any tensor.
 *
 * bincode 1.3 as the free functions serialize / deserialize use it: fixed-width
 * little-endian integers, an enum variant is a u32, a Vec length a u64, a bool
 * one byte that must be 0 or 1, an i8 one byte, a u128 16 bytes.  A datagram is
 * magic u16, variant u32, then
 *   0 SyncRequest     u32
 *   1 SyncReply       u32
 *   2 Input           u64 n, n x (bool disconnected, i32 last_frame),
 *                     bool disconnect_requested, i32 start_frame, i32 ack_frame,
 *                     u64 len, len bytes
 *   3 InputAck        i32 ack_frame
 *   4 QualityReport   i8 frame_advantage, u128 ping
 *   5 QualityReply    u128 pong
 *   6 ChecksumReport  u128 checksum, i32 frame
 *   7 KeepAlive
 * Trailing bytes are accepted; a short buffer, a variant above 7, a bool above 1
 * or a length that runs past the buffer is malformed, and the reference's socket
 * drops such a datagram before handle_message sees it (udp_socket.rs:42).
 *
 * Status bits, int32 [P][S], written by every call for every endpoint served: */
#define RB_DG_MALFORMED 1         /* parse: a datagram bincode refuses, or an Input with n != num_players */
#define RB_DG_MAGIC_MISMATCH 2    /* parse: dropped by protocol.rs:551 */
#define RB_DG_SYNC_SEEN 4         /* parse: a SyncRequest / SyncReply came; it stamps `received`; rb_endpoint_protocol_poll_all answers it */
#define RB_DG_BAD_PONG 8          /* parse: a QualityReply from the future, or a round trip beyond int32 */
#define RB_DG_REPORTS_DROPPED 16  /* parse: more than RB_P2P_REPORTS_PER_TAKE reports were pending */
#define RB_DG_NO_ROOM 32          /* build: a message did not fit the slots or the stride and was left out */
#define RB_DG_ADVANTAGE_RANGE 64  /* build: frame_advantage outside i8; no QualityReport (the reference panics, protocol.rs:519-520) */
#define RB_DG_MAX_SLOTS 8

/* UdpProtocol::handle_message (protocol.rs:544-575) with on_input's head
 * (:616-637), on_input_ack (:692-694), on_quality_report / on_quality_reply
 * (:697-708) and the collecting half of on_checksum_report (:710-722) for every
 * endpoint: the datagrams the caller's sockets collected since the last call, in
 * up to RB_DG_MAX_SLOTS slots per endpoint, handled in slot order.  Every
 * pointer is device memory and none may be NULL.
 *   datagrams        uint8 [slots][P*S][stride], 16-byte aligned; stride a
 *                    multiple of 16 of at least 64
 *   dg_lengths       int32 [slots][P][S]; 0 or negative: an empty slot.  No byte
 *                    at or above min(length, stride) decides anything
 *   remote_magic     uint16 [P][S]; 0 accepts any magic (:551)
 *   now_ms           the caller's epoch clock, >= 0 (millis_since_epoch)
 * For each datagram accepted (well formed, magic right):
 *   received         uint8 [P][S] = 1, else 0: rb_p2p_poll_liveness's tensor
 *   Input            acked (in/out int32 [P][S]) = max(acked, ack_frame);
 *                    disconnect_requested (uint8 [P][S], 0 otherwise) |= flag;
 *                    with the flag clear the status vector is merged into
 *                    peer_last_frames int32 [P endpoints][P players][S] (max,
 *                    from RB_NULL_FRAME) and peer_disconnected uint8, same shape
 *                    (OR, from 0), over this call's messages: the merge is
 *                    monotone, so rb_p2p_receive_peer_connect_status(h, row h)
 *                    equals applying each message in turn (:627-636).  An Input
 *                    whose n is not num_players is malformed (the reference
 *                    indexes past a short vector and panics).  The payload of
 *                    the last Input in slot order goes to packets / lengths /
 *                    start_frames in rb_decode_input_packets_all's layout
 *                    (lengths 0: none; bytes of the row past the payload are
 *                    unspecified); earlier Inputs of the call count as lost
 *                    datagrams for their payload only, and the sender repeats
 *                    what was not acknowledged.  A payload longer than
 *                    packet_stride leaves its true length and its first
 *                    packet_stride bytes: the decoder refuses that length.
 *   InputAck         acked = max(acked, ack_frame)
 *   QualityReport    frame_advantage (in/out int32 [P][S]) takes the value,
 *                    reply_owed uint8 [P][S] = 1 (else 0) and reply_ping
 *                    uint64 [2 lo, hi][P][S] the u128 to echo (else 0); the last
 *                    report wins
 *   QualityReply     rtt_ms (in/out int32 [P][S]) = now_ms - pong; a pong above
 *                    now_ms (the reference asserts, :706) or a difference beyond
 *                    int32 leaves rtt_ms and sets RB_DG_BAD_PONG
 *   ChecksumReport   appended to reports [P][RB_P2P_REPORTS_PER_TAKE][S]
 *                    rb_checksum_report behind the report_counts (in/out int32
 *                    [P][S]) entries already there; handle h's slice is what
 *                    rb_p2p_receive_checksum_reports(h, slice,
 *                    RB_P2P_REPORTS_PER_TAKE) takes, after which the caller
 *                    zeroes report_counts[h].  Entries at and above the count
 *                    are written RB_NULL_FRAME (mismatch_frame RB_NULL_FRAME,
 *                    checksum 0) by every call.  Beyond the capacity the oldest
 *                    leave and RB_DG_REPORTS_DROPPED is set.
 *   SyncRequest / SyncReply   RB_DG_SYNC_SEEN, nothing else
 * RB_INVALID_REQUEST, with nothing launched and no tensor touched: an empty mask
 * or bits at or above num_players; num_players > 4; slots outside
 * 1..RB_DG_MAX_SLOTS; a stride or packet_stride that breaks the rules above /
 * of rb_decode_input_packets_all, or a misaligned datagrams / packets pointer;
 * now_ms < 0; a NULL pointer. */
typedef struct rb_datagram_parse {
  const uint8_t* datagrams;
  int64_t stride;
  int32_t slots;
  int32_t reserved;
  const int32_t* dg_lengths;
  const uint16_t* remote_magic;
  int64_t now_ms;
  uint8_t* received;
  uint8_t* disconnect_requested;
  int32_t* acked;
  int32_t* peer_last_frames;
  uint8_t* peer_disconnected;
  uint8_t* packets;
  int64_t packet_stride;
  int32_t* lengths;
  int32_t* start_frames;
  int32_t* frame_advantage;
  uint8_t* reply_owed;
  uint64_t* reply_ping;
  int32_t* rtt_ms;
  rb_checksum_report* reports;
  int32_t* report_counts;
  int32_t* status;
} rb_datagram_parse;
rb_status rb_parse_datagrams_all(int32_t device, void* stream, uint32_t handle_mask, int32_t num_players,
                                 int32_t num_sessions, const rb_datagram_parse* io);

/* The messages every endpoint owes this poll, as queue_message's callers build
 * them (protocol.rs:468-525, 736-742), packed densely per endpoint in this
 * order into out_datagrams uint8 [slots][P*S][stride] (16-byte aligned, stride
 * as above), their lengths in out_lengths int32 [slots][P][S] (0: an empty
 * slot; bytes of a row past the length are unspecified) and their number in
 * out_counts int32 [P][S]:
 *   1. Input, where lengths > 0: the packet rb_encode_input_packets_all wrote
 *      (packets / packet_stride / lengths / start_frames), ack_frame (int32
 *      [P][S]: the `upto` row, last_recv_frame), disconnect_requested (uint8
 *      [P][S]) and the sender's connect status, status_last_frames int32 /
 *      status_disconnected uint8 [P players][S] (:468-492).  A length above
 *      packet_stride is no packet: RB_DG_MALFORMED, no Input.
 *   2. InputAck{ack_frame}, where ack_owed uint8 [P][S] is set (:495-501)
 *   3. QualityReply, where reply_owed is set, echoing reply_ping (the tensors
 *      rb_parse_datagrams_all wrote)
 *   4. QualityReport, where report_due uint8 [P][S] is set (:516-525):
 *      frame_advantage int32 [P][S] is the local_adv row of
 *      rb_p2p_export_time_sync (outside i8: RB_DG_ADVANTAGE_RANGE and no
 *      message); ping = now_ms
 *   5. a ChecksumReport for every entry of reports [RB_P2P_REPORTS_PER_TAKE][S]
 *      (rb_p2p_take_checksum_reports' tensor) whose frame is not RB_NULL_FRAME,
 *      the same for every endpoint of a session (:736-742)
 *   6. KeepAlive, where keepalive_due uint8 [P][S] is set and nothing else was
 *      written for the endpoint
 * A message that does not fit the slots left or the stride is left out and sets
 * RB_DG_NO_ROOM; the ones after it are still tried.  local_magic is uint16
 * [P][S].  Which bytes are due is decided outside this call: by
 * rb_endpoint_protocol_poll_all, below (the 200 ms send timers), whose outputs
 * are this call's lengths, ack_owed, reply_owed, report_due and keepalive_due,
 * or by the caller's own timers.  NULL means "none due" for packets (with lengths and
 * start_frames), disconnect_requested, ack_owed, reply_owed (with reply_ping),
 * report_due (with frame_advantage), reports and keepalive_due; the other
 * pointers may not be NULL.  RB_INVALID_REQUEST as for rb_parse_datagrams_all. */
typedef struct rb_datagram_build {
  const uint16_t* local_magic;
  int64_t now_ms;
  const uint8_t* packets;
  int64_t packet_stride;
  const int32_t* lengths;
  const int32_t* start_frames;
  const int32_t* ack_frame;
  const uint8_t* disconnect_requested;
  const int32_t* status_last_frames;
  const uint8_t* status_disconnected;
  const uint8_t* ack_owed;
  const uint8_t* reply_owed;
  const uint64_t* reply_ping;
  const uint8_t* report_due;
  const int32_t* frame_advantage;
  const rb_checksum_report* reports;
  const uint8_t* keepalive_due;
  uint8_t* out_datagrams;
  int64_t stride;
  int32_t slots;
  int32_t reserved;
  int32_t* out_lengths;
  int32_t* out_counts;
  int32_t* status;
} rb_datagram_build;
rb_status rb_build_datagrams_all(int32_t device, void* stream, uint32_t handle_mask, int32_t num_players,
                                 int32_t num_sessions, const rb_datagram_build* io);

/* ---- UdpProtocol's handshake, state machine and send timers for every endpoint
 * of a batch in one launch: the part of
 * network/protocol.rs that decides which message is due and when.  Stateless in
 * the library like the two calls above and laid out like them: the endpoint of
 * handle h, session s is row h*S + s of every [P][S] tensor, handle_mask selects
 * the handles served, and no row of a handle outside it is touched, in any
 * tensor.  The endpoint's state lives in the caller's tensors; a fresh endpoint
 * is all zero bytes in every one of them, so restarting a session's endpoints
 * means zeroing their columns.  ProtocolState (protocol.rs:119-125): */
#define RB_EP_INITIALIZING 0
#define RB_EP_SYNCHRONIZING 1
#define RB_EP_RUNNING 2
#define RB_EP_DISCONNECTED 3
#define RB_EP_SHUTDOWN 4 /* and any byte above it: an unknown state is never run and never written */
#define RB_EP_EVENT_SYNCHRONIZING 1 /* events bit 0: Event::Synchronizing{total 5, count sync_count} (:599-603) */
#define RB_EP_EVENT_SYNCHRONIZED 2  /* events bit 1: Event::Synchronized (:610) */
#define RB_EP_STAMPS 5 /* last_send, last_input_recv, last_quality_report, shutdown_at, stats_start */

/* State, in/out, device memory, none NULL:
 *   ep_state        uint8 [P][S]     RB_EP_* (UdpProtocol::state)
 *   sync_remaining  int32 [P][S]     sync_remaining_roundtrips (:138)
 *   sync_nonces     uint32 [8][P][S] sync_random_requests (:139), the newest 8
 *                   outstanding nonces: the reference's HashSet grows without
 *                   bound; here a reply to a request more than 8 requests old
 *                   is ignored and the handshake goes on with the newer ones.
 *                   Inserting a value that is already valid adds nothing, as a
 *                   set does (the request is still sent, :507-514)
 *   sync_valid      uint8 [P][S]     bit i: entry i of sync_nonces is outstanding
 *   sync_next       uint8 [P][S]     the entry the next insert writes (read & 7)
 *   stamps          int64 [RB_EP_STAMPS][P][S], the caller's milliseconds:
 *                   last_send_time (:173), running_last_input_recv (:141),
 *                   running_last_quality_report (:140), shutdown_timeout (:148),
 *                   stats_start_time (:169)
 *   packets_sent    int64 [P][S]     messages declared due so far (:170, :532)
 *   last_newest     int32 [P][S]     1 + the newest local frame an Input was
 *                   already declared due for (0: none, so that a zeroed row is
 *                   an endpoint that has sent nothing)
 *   remote_magic    uint16 [P][S]    the tensor rb_parse_datagrams_all takes;
 *                   written here when the handshake ends (:612)
 * Inputs; "optional" may be NULL, meaning none or zero:
 *   now_ms          the caller's clock, >= 0
 *   local_magic     uint16 [P][S]    UdpProtocol::magic (:198-201)
 *   start           uint8 [P][S], optional: synchronize() (:335-341)
 *   datagrams, stride, slots, dg_lengths: the tensors handed to
 *                   rb_parse_datagrams_all.  Only variants 0 and 1 are read.
 *                   stride a multiple of 16 of at least 16, the tensor 16-byte
 *                   aligned
 *   nonces          uint32 [slots][P][S]: rand::random::<u32>() is the caller's
 *                   (:508).  The j-th SyncRequest an endpoint sends in this call
 *                   uses nonces[j]; a request beyond the slots-th is not sent
 *                   (RB_DG_NO_ROOM)
 *   disconnected    uint8 [P][S], optional: bit 2 of rb_p2p_poll_liveness's
 *                   state_out, or any non-zero byte: disconnect() (:325-333)
 *   ack_owed        uint8 [P][S], optional: set where this poll's decode
 *                   accepted an Input (the byte rb_build_datagrams_all takes)
 *   reply_owed, received  rb_parse_datagrams_all's tensors, optional
 *   newest          int32 [P][S]: the sent tensor of rb_p2p_export_local_inputs
 *   acked           int32 [P][S]: rb_parse_datagrams_all's in/out tensor
 *   lengths         int32 [P][S], optional: rb_encode_input_packets_all's output
 *   reports         [RB_P2P_REPORTS_PER_TAKE][S], optional:
 *                   rb_build_datagrams_all's tensor, read once per session
 * Outputs, each written for every endpoint served:
 *   input_lengths   int32 [P][S] = lengths where an Input is due, else 0: hand
 *                   it to rb_build_datagrams_all as lengths
 *   ack_due, reply_due, report_due, keepalive_due  uint8 [P][S]: that call's
 *                   ack_owed / reply_owed / report_due / keepalive_due
 *   sync_datagrams  uint8 [sync_slots][P*S][stride], sync_lengths int32
 *                   [sync_slots][P][S] (10 or 0), sync_counts int32 [P][S]: the
 *                   SyncRequests and SyncReplies, in rb_build_datagrams_all's
 *                   layout with the same stride (bytes past the length are zero
 *                   up to byte 15; rows at and above the count are untouched)
 *   events          uint8 [P][S] RB_EP_EVENT_*; several Synchronizing events of
 *                   one call fold into one bit with the newest count
 *   sync_count      int32 [P][S] = NUM_SYNC_PACKETS - sync_remaining after the call
 *   liveness_received  uint8 [P][S], optional = received | (ep_state != RUNNING)
 *                   after the call: rb_p2p_poll_liveness's `received`.  poll's
 *                   receive timers run in Running only (:360, :377-394), so an
 *                   endpoint in any other state never ages
 *   send_queue_len  int32 [P][S], optional = pending_output.len() (:296) =
 *                   max(0, newest - acked); acked RB_NULL_FRAME counts from frame 0
 *   session_running uint8 [S], optional = 1 where every endpoint of the mask
 *                   is_synchronized() (:307-311; p2p_session.rs:598-618): the
 *                   run mask rb_p2p_run_ticks_paced takes
 *   status          int32 [P][S]: RB_DG_NO_ROOM where a sync message found no slot
 *
 * Per endpoint and call, in this order:
 *  1. SHUTDOWN: nothing is read, every send output, events, sync_count,
 *     send_queue_len and status is 0, liveness_received 1, the state untouched
 *     (:429-432, :546-548).
 *  2. disconnected set while the state is neither DISCONNECTED nor SHUTDOWN: the
 *     state becomes DISCONNECTED and shutdown_at = now + 5000 (:325-333).
 *  3. start set while INITIALIZING is synchronize() (:335-341): SYNCHRONIZING,
 *     sync_remaining = 5, stats_start = now, one SyncRequest.  last_send,
 *     last_input_recv and last_quality_report are set to now; the reference
 *     stamps them at construction (:226-260), a deviation of at most the gap
 *     between construction and synchronize, as section 18 states for its own.
 *  4. Every slot in slot order: a datagram with at least 10 bytes below
 *     min(length, stride) and variant 0 or 1 that passes the magic filter
 *     (remote_magic != 0 && magic != remote_magic drops it, :551, with the value
 *     as earlier slots of this call left it).  SyncRequest{x} queues
 *     SyncReply{x} in any state (:578-583).  SyncReply{x} is on_sync_reply
 *     (:586-614): ignored unless SYNCHRONIZING and x is outstanding; else the
 *     nonce leaves and sync_remaining -= 1; above 0 that raises events bit 0
 *     and sends another SyncRequest, at 0 the state becomes RUNNING, events bit
 *     1 is raised and remote_magic takes the datagram's magic.
 *  5. ack_owed sets ack_due and last_input_recv = now (:654, :682); reply_owed
 *     sets reply_due (:697-701).
 *  6. poll's timers (:351-404), all strict `<` in 64 bits.  SYNCHRONIZING:
 *     last_send + 200 < now sends a SyncRequest.  RUNNING: last_input_recv + 200
 *     < now sets the stamp to now, and an Input is due if newest > acked
 *     (pending_output has a front, :468-471); last_quality_report + 200 < now
 *     sets report_due and the stamp.  DISCONNECTED: shutdown_at < now makes the
 *     state SHUTDOWN, and every send output of this call is 0 and nothing is
 *     counted: the queue is drained before the socket sees it (:429-432).
 *     queue_message stamps last_send_time at once (:533), so last_send reads as
 *     now wherever this call already declared a message due.
 *  7. The frame's own sends.  In RUNNING only (:444-446) newest above the last
 *     frame sent makes an Input due; in every state last_newest follows newest,
 *     so an input that arrived while the endpoint was not running is not sent
 *     late on its own: it travels with the resend timer or the next frame.  One
 *     Input is one message however many reasons it has.  Each entry of reports
 *     whose frame is not RB_NULL_FRAME counts as one message (:736-742).
 *  8. KeepAlive (:372-375): RUNNING, nothing declared due in steps 3-7 and
 *     last_send + 200 < now.  One call folds one poll_remote_clients and the
 *     frame's sends that follow it, so a KeepAlive the reference would queue
 *     just ahead of an Input of the same iteration is not sent:
 *     rb_build_datagrams_all's rule 6.
 *  9. packets_sent rises by the messages declared due, sync messages included;
 *     above 0, last_send = now (:527-538).  A sync message that finds no slot
 *     is not sent and not counted, a request's nonce is not recorded, and
 *     RB_DG_NO_ROOM is set; the 200 ms retry repeats it.
 * Sync messages leave in the order "replies and requests as handled, then the
 * timer's request".  disconnect_requested is never set on an outgoing Input and
 * has no output here: the reference cannot send it either, send_pending_output
 * runs in Running only while the flag is state == Disconnected (:488).  The
 * pending-output overflow disconnect (:461-463) and spectator endpoints are out
 * of scope.  kbps_sent (:279-301) adds size_of_val(&msg), a constant of the
 * reference's build, per message; the caller computes
 * ((packets_sent * (message_bytes + 28)) / seconds) / 1024 with seconds =
 * (now - stats_start) / 1000 from the two state rows, NotSynchronized where
 * seconds == 0 or the state is neither SYNCHRONIZING nor RUNNING.
 *
 * RB_INVALID_REQUEST, with nothing launched and no tensor touched: an empty mask
 * or bits at or above num_players; num_players > 4; slots or sync_slots outside
 * 1..RB_DG_MAX_SLOTS; a stride that breaks the rule above or is beyond 1 MiB,
 * or a misaligned
 * datagrams / sync_datagrams pointer; now_ms < 0; a NULL pointer that is not
 * optional. */
typedef struct rb_endpoint_protocol {
  /* state */
  uint8_t* ep_state;
  int32_t* sync_remaining;
  uint32_t* sync_nonces;
  uint8_t* sync_valid;
  uint8_t* sync_next;
  int64_t* stamps;
  int64_t* packets_sent;
  int32_t* last_newest;
  uint16_t* remote_magic;
  /* inputs */
  int64_t now_ms;
  const uint16_t* local_magic;
  const uint8_t* start;
  const uint8_t* datagrams;
  int64_t stride;
  int32_t slots;
  int32_t sync_slots;
  const int32_t* dg_lengths;
  const uint32_t* nonces;
  const uint8_t* disconnected;
  const uint8_t* ack_owed;
  const uint8_t* reply_owed;
  const uint8_t* received;
  const int32_t* newest;
  const int32_t* acked;
  const int32_t* lengths;
  const rb_checksum_report* reports;
  /* outputs */
  int32_t* input_lengths;
  uint8_t* ack_due;
  uint8_t* reply_due;
  uint8_t* report_due;
  uint8_t* keepalive_due;
  uint8_t* sync_datagrams;
  int32_t* sync_lengths;
  int32_t* sync_counts;
  uint8_t* events;
  int32_t* sync_count;
  uint8_t* liveness_received;
  int32_t* send_queue_len;
  uint8_t* session_running;
  int32_t* status;
} rb_endpoint_protocol;
rb_status rb_endpoint_protocol_poll_all(int32_t device, void* stream, uint32_t handle_mask, int32_t num_players,
                                        int32_t num_sessions, const rb_endpoint_protocol* io);

#ifdef __cplusplus
} /* extern "C" */
#endif
#endif /* GGRS_AMD_H */
