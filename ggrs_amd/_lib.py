"""ctypes binding of libggrs_amd.so (include/ggrs_amd.h).

The shared library is built in-tree by ``ggrs_amd/csrc/Makefile`` (see
``__graft_entry__.build``).  There is no fallback: importing this module
without the library raises, so nothing can silently run on the CPU.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# GGRS_AMD_LIB: load another build of the same library (kernel experiments, tools/)
LIB_PATH = os.environ.get("GGRS_AMD_LIB") or os.path.join(_HERE, "libggrs_amd.so")

RB_ABI_VERSION = 1
RB_NULL_FRAME = -1
RB_INPUT_QUEUE_LENGTH = 128  # input_queue.rs:6

# rb_status
RB_OK = 0
RB_PREDICTION_THRESHOLD = 1
RB_INVALID_REQUEST = 2
RB_MISMATCHED_CHECKSUM = 3
RB_NOT_SYNCHRONIZED = 4
RB_SPECTATOR_TOO_FAR_BEHIND = 5
RB_DEVICE_ERROR = 100
RB_PANIC = 101

# rb_game
RB_GAME_EX_GAME = 1
RB_GAME_STUB = 2
RB_GAME_STUB_ENUM = 3
RB_GAME_STUB_RANDOM_CS = 4
RB_GAME_BRAWLER = 5

RB_FLAG_CHECKED = 1
RB_FLAG_LANE_PER_SESSION = 2
RB_P2P_FLAG_FANOUT = 4
RB_P2P_FLAG_PEER_STATUS = 8
RB_P2P_FLAG_FANOUT_ALWAYS = 16
RB_P2P_FLAG_FANOUT_PER_PLAYER = 32
RB_GAME_PLUGIN_BASE = 1000
RB_P2P_REPORTS_PER_TAKE = 8
RB_P2P_EVENTS_KEPT = 16
RB_P2P_WAIT_EVENTS_KEPT = 8
RB_P2P_NET_EVENTS_KEPT = 16
RB_NET_INTERRUPTED, RB_NET_RESUMED, RB_NET_DISCONNECTED = 1, 2, 3
RB_DG_MALFORMED, RB_DG_MAGIC_MISMATCH, RB_DG_SYNC_SEEN, RB_DG_BAD_PONG, RB_DG_REPORTS_DROPPED = 1, 2, 4, 8, 16
RB_DG_NO_ROOM, RB_DG_ADVANTAGE_RANGE = 32, 64
RB_DG_MAX_SLOTS = 8
RB_EP_INITIALIZING, RB_EP_SYNCHRONIZING, RB_EP_RUNNING, RB_EP_DISCONNECTED, RB_EP_SHUTDOWN = 0, 1, 2, 3, 4
RB_EP_EVENT_SYNCHRONIZING, RB_EP_EVENT_SYNCHRONIZED = 1, 2
RB_EP_STAMPS = 5
RB_P2P_EXPORT_OK = 0
RB_P2P_EXPORT_OVERRUN = 1
SPECTATOR_BUFFER_SIZE = 60  # p2p_spectator_session.rs:16


class RbConfig(ctypes.Structure):
    _fields_ = [
        ("abi_version", ctypes.c_int32),
        ("game", ctypes.c_int32),
        ("num_sessions", ctypes.c_int32),
        ("num_players", ctypes.c_int32),
        ("max_prediction", ctypes.c_int32),
        ("check_distance", ctypes.c_int32),
        ("input_delay", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("seed", ctypes.c_uint64),
        ("flags", ctypes.c_uint32),
        ("block_size", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32 * 6),
    ]


class RbP2PConfig(ctypes.Structure):
    _fields_ = [
        ("abi_version", ctypes.c_int32),
        ("game", ctypes.c_int32),
        ("num_sessions", ctypes.c_int32),
        ("num_players", ctypes.c_int32),
        ("max_prediction", ctypes.c_int32),
        ("input_delay", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("local_mask", ctypes.c_uint32),
        ("remote_delay", ctypes.c_int32),
        ("sparse_saving", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("block_size", ctypes.c_uint32),
        ("desync_interval", ctypes.c_int32),
        ("fanout_candidates", ctypes.c_int32),
        ("fanout_min_select_permille", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32 * 1),
    ]


class RbSpectatorConfig(ctypes.Structure):
    _fields_ = [
        ("abi_version", ctypes.c_int32),
        ("game", ctypes.c_int32),
        ("num_sessions", ctypes.c_int32),
        ("num_players", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("max_frames_behind", ctypes.c_int32),
        ("catchup_speed", ctypes.c_int32),
        ("block_size", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32 * 4),
    ]


class RbChecksumReport(ctypes.Structure):
    _fields_ = [
        ("checksum_lo", ctypes.c_uint64),
        ("checksum_hi", ctypes.c_uint64),
        ("frame", ctypes.c_int32),
        ("mismatch_frame", ctypes.c_int32),
    ]


class RbDatagramParse(ctypes.Structure):
    _fields_ = [
        ("datagrams", ctypes.c_void_p),
        ("stride", ctypes.c_int64),
        ("slots", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("dg_lengths", ctypes.c_void_p),
        ("remote_magic", ctypes.c_void_p),
        ("now_ms", ctypes.c_int64),
        ("received", ctypes.c_void_p),
        ("disconnect_requested", ctypes.c_void_p),
        ("acked", ctypes.c_void_p),
        ("peer_last_frames", ctypes.c_void_p),
        ("peer_disconnected", ctypes.c_void_p),
        ("packets", ctypes.c_void_p),
        ("packet_stride", ctypes.c_int64),
        ("lengths", ctypes.c_void_p),
        ("start_frames", ctypes.c_void_p),
        ("frame_advantage", ctypes.c_void_p),
        ("reply_owed", ctypes.c_void_p),
        ("reply_ping", ctypes.c_void_p),
        ("rtt_ms", ctypes.c_void_p),
        ("reports", ctypes.c_void_p),
        ("report_counts", ctypes.c_void_p),
        ("status", ctypes.c_void_p),
    ]


class RbDatagramBuild(ctypes.Structure):
    _fields_ = [
        ("local_magic", ctypes.c_void_p),
        ("now_ms", ctypes.c_int64),
        ("packets", ctypes.c_void_p),
        ("packet_stride", ctypes.c_int64),
        ("lengths", ctypes.c_void_p),
        ("start_frames", ctypes.c_void_p),
        ("ack_frame", ctypes.c_void_p),
        ("disconnect_requested", ctypes.c_void_p),
        ("status_last_frames", ctypes.c_void_p),
        ("status_disconnected", ctypes.c_void_p),
        ("ack_owed", ctypes.c_void_p),
        ("reply_owed", ctypes.c_void_p),
        ("reply_ping", ctypes.c_void_p),
        ("report_due", ctypes.c_void_p),
        ("frame_advantage", ctypes.c_void_p),
        ("reports", ctypes.c_void_p),
        ("keepalive_due", ctypes.c_void_p),
        ("out_datagrams", ctypes.c_void_p),
        ("stride", ctypes.c_int64),
        ("slots", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("out_lengths", ctypes.c_void_p),
        ("out_counts", ctypes.c_void_p),
        ("status", ctypes.c_void_p),
    ]


class RbEndpointProtocol(ctypes.Structure):
    _fields_ = [
        ("ep_state", ctypes.c_void_p),
        ("sync_remaining", ctypes.c_void_p),
        ("sync_nonces", ctypes.c_void_p),
        ("sync_valid", ctypes.c_void_p),
        ("sync_next", ctypes.c_void_p),
        ("stamps", ctypes.c_void_p),
        ("packets_sent", ctypes.c_void_p),
        ("last_newest", ctypes.c_void_p),
        ("remote_magic", ctypes.c_void_p),
        ("now_ms", ctypes.c_int64),
        ("local_magic", ctypes.c_void_p),
        ("start", ctypes.c_void_p),
        ("datagrams", ctypes.c_void_p),
        ("stride", ctypes.c_int64),
        ("slots", ctypes.c_int32),
        ("sync_slots", ctypes.c_int32),
        ("dg_lengths", ctypes.c_void_p),
        ("nonces", ctypes.c_void_p),
        ("disconnected", ctypes.c_void_p),
        ("ack_owed", ctypes.c_void_p),
        ("reply_owed", ctypes.c_void_p),
        ("received", ctypes.c_void_p),
        ("newest", ctypes.c_void_p),
        ("acked", ctypes.c_void_p),
        ("lengths", ctypes.c_void_p),
        ("reports", ctypes.c_void_p),
        ("input_lengths", ctypes.c_void_p),
        ("ack_due", ctypes.c_void_p),
        ("reply_due", ctypes.c_void_p),
        ("report_due", ctypes.c_void_p),
        ("keepalive_due", ctypes.c_void_p),
        ("sync_datagrams", ctypes.c_void_p),
        ("sync_lengths", ctypes.c_void_p),
        ("sync_counts", ctypes.c_void_p),
        ("events", ctypes.c_void_p),
        ("sync_count", ctypes.c_void_p),
        ("liveness_received", ctypes.c_void_p),
        ("send_queue_len", ctypes.c_void_p),
        ("session_running", ctypes.c_void_p),
        ("status", ctypes.c_void_p),
    ]


# Every symbol declared in include/ggrs_amd.h: (name, restype, argtypes).
_P = ctypes.c_void_p
_I32 = ctypes.c_int32
_PI32 = ctypes.POINTER(ctypes.c_int32)
_PU64 = ctypes.POINTER(ctypes.c_uint64)
SIGNATURES = [
    ("rb_config_init", None, [ctypes.POINTER(RbConfig)]),
    ("rb_synctest_create", _I32, [ctypes.POINTER(RbConfig), ctypes.POINTER(_P)]),
    ("rb_destroy", None, [_P]),
    ("rb_last_error", ctypes.c_char_p, [_P]),
    ("rb_set_stream", _I32, [_P, _P]),
    ("rb_get_stream", _P, [_P]),
    ("rb_add_local_input", _I32, [_P, _I32, _P, _I32]),
    ("rb_add_local_inputs_packed", _I32, [_P, _P, _I32]),
    ("rb_advance_frame", _I32, [_P]),
    ("rb_run_ticks", _I32, [_P, _I32, _P, ctypes.c_int64, _I32, _PI32]),
    ("rb_current_frame", _I32, [_P]),
    ("rb_num_sessions", _I32, [_P]),
    ("rb_state_bytes", _I32, [_P]),
    ("rb_input_bytes", _I32, [_P]),
    ("rb_synchronize", _I32, [_P]),
    ("rb_mismatches", _I32, [_P, _PI32, _PI32]),
    ("rb_last_requests", _I32, [_P, _PI32, _PI32, _I32]),
    ("rb_read_cell", _I32, [_P, _I32, _P, _PU64]),
    ("rb_read_live", _I32, [_P, _P, _PU64, _PI32]),
    ("rb_export_checksum_report", _I32, [_P, _I32, _P]),
    ("rb_export_compact_report", _I32, [_P, _I32, _P]),
    ("rb_p2p_fanout_state", _I32, [_P, _PI32, ctypes.POINTER(ctypes.c_double), _PI32, _PI32]),
    ("rb_debug_corrupt_cell", _I32, [_P, _I32, _I32, _I32, ctypes.c_uint32]),
    ("rb_debug_sincosf", _I32, [_I32, _P, _P, _P, ctypes.c_int64]),
    ("rb_debug_speed_clamp", _I32, [_I32, _P, _P, _P, _P, ctypes.c_int64]),
    ("rb_debug_exgame_inrange", _I32, [_I32, ctypes.c_uint32, ctypes.c_int64, _P]),
    ("rb_debug_exgame_position_clamp", _I32, [_I32, ctypes.c_uint32, ctypes.c_int64, _PU64, _P]),
    ("rb_profile_enable", _I32, [_P, _I32]),
    ("rb_profile_take", _I32, [_P, ctypes.POINTER(ctypes.c_double), _PI32]),
    ("rb_launch_clock_arm", _I32, [_P, _I32]),
    ("rb_launch_clock_read", _I32, [_P, _PU64, _I32, _PI32]),
    ("rb_register_game_plugin", _I32, [ctypes.c_char_p, _PI32]),
    ("rb_p2p_config_init", None, [ctypes.POINTER(RbP2PConfig)]),
    ("rb_p2p_create", _I32, [ctypes.POINTER(RbP2PConfig), ctypes.POINTER(_P)]),
    ("rb_p2p_destroy", None, [_P]),
    ("rb_p2p_last_error", ctypes.c_char_p, [_P]),
    ("rb_p2p_set_stream", _I32, [_P, _P]),
    ("rb_p2p_get_stream", _P, [_P]),
    ("rb_p2p_run_ticks", _I32, [_P, _I32, _P, ctypes.c_int64, _P, _P, _I32]),
    ("rb_p2p_run_ticks_packets", _I32, [_P, _I32, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P, _P]),
    ("rb_p2p_read_status", _I32, [_P, _P, _P, _P, _P]),
    ("rb_p2p_disconnect_player", _I32, [_P, _I32, _P]),
    ("rb_p2p_restart_sessions", _I32, [_P, _P]),
    ("rb_p2p_export_sessions", _I32, [_P, _P, _I32, _P]),
    ("rb_p2p_import_sessions", _I32, [_P, _P, _I32, _P]),
    ("rb_p2p_import_refused", _I32, [_P, _P]),
    ("rb_p2p_read_frames", _I32, [_P, _P, _P]),
    ("rb_p2p_read_queues", _I32, [_P, _P]),
    ("rb_p2p_read_cells", _I32, [_P, _P, _P, _P]),
    ("rb_p2p_read_live", _I32, [_P, _P]),
    ("rb_p2p_state_bytes", _I32, [_P]),
    ("rb_p2p_input_bytes", _I32, [_P]),
    ("rb_p2p_counters", _I32, [_P, _P]),
    ("rb_p2p_totals", _I32, [_P, _P]),
    ("rb_p2p_take_checksum_reports", _I32, [_P, _P]),
    ("rb_p2p_receive_checksum_reports", _I32, [_P, _I32, _P, _I32]),
    ("rb_p2p_read_desync_events", _I32, [_P, _P, _P, _P, _P, _P]),
    ("rb_p2p_debug_corrupt", _I32, [_P, _I32, _I32, ctypes.c_uint32]),
    ("rb_p2p_receive_peer_connect_status", _I32, [_P, _I32, _P, _P]),
    ("rb_p2p_export_confirmed_inputs", _I32, [_P, _P, _I32, _P, _P, _P]),
    ("rb_p2p_read_export_status", _I32, [_P, _P, _P]),
    ("rb_p2p_set_delivery_ring", _I32, [_P, _I32]),
    ("rb_p2p_export_local_inputs", _I32, [_P, _P, _I32, _P]),
    ("rb_p2p_time_sync_enable", _I32, [_P, _I32]),
    ("rb_p2p_receive_quality", _I32, [_P, _I32, _P, _P]),
    ("rb_p2p_export_time_sync", _I32, [_P, _P, _P]),
    ("rb_p2p_read_time_sync", _I32, [_P, _P, _P, _P, _P]),
    ("rb_p2p_read_wait_recommendations", _I32, [_P, _P, _P, _P]),
    ("rb_p2p_debug_read_time_sync_windows", _I32, [_P, _P]),
    ("rb_p2p_run_ticks_paced", _I32, [_P, _I32, _P, ctypes.c_int64, _P, _P, _I32, _P]),
    ("rb_p2p_pace", _I32, [_P, _P]),
    ("rb_p2p_read_pacing", _I32, [_P, _P]),
    ("rb_p2p_liveness_enable", _I32, [_P, _I32, _I32]),
    ("rb_p2p_poll_liveness", _I32, [_P, ctypes.c_int64, _P, _P, _P]),
    ("rb_p2p_read_network_events", _I32, [_P, _P, _P, _P, _P]),
    ("rb_p2p_read_liveness", _I32, [_P, _P, _P]),
    ("rb_debug_time_sync_average", _I32, [_I32, _P, _P, _P, ctypes.c_int64]),
    ("rb_p2p_profile_enable", _I32, [_P, _I32]),
    ("rb_p2p_profile_take", _I32, [_P, ctypes.POINTER(ctypes.c_double), _PI32]),
    ("rb_p2p_launch_clock_arm", _I32, [_P, _I32]),
    ("rb_p2p_launch_clock_read", _I32, [_P, _PU64, _I32, _PI32]),
    ("rb_spectator_config_init", None, [ctypes.POINTER(RbSpectatorConfig)]),
    ("rb_spectator_create", _I32, [ctypes.POINTER(RbSpectatorConfig), ctypes.POINTER(_P)]),
    ("rb_spectator_destroy", None, [_P]),
    ("rb_spectator_last_error", ctypes.c_char_p, [_P]),
    ("rb_spectator_set_stream", _I32, [_P, _P]),
    ("rb_spectator_get_stream", _P, [_P]),
    ("rb_spectator_receive_host_status", _I32, [_P, _P, _P]),
    ("rb_spectator_restart_sessions", _I32, [_P, _P]),
    ("rb_spectator_export_sessions", _I32, [_P, _P, _I32, _P]),
    ("rb_spectator_import_sessions", _I32, [_P, _P, _I32, _P]),
    ("rb_spectator_import_refused", _I32, [_P, _P]),
    ("rb_spectator_run_ticks", _I32, [_P, _I32, _P, _P, _I32]),
    ("rb_spectator_set_delivery_ring", _I32, [_P, _I32]),
    ("rb_spectator_read_status", _I32, [_P, _P, _P]),
    ("rb_spectator_read_frames", _I32, [_P, _P, _P]),
    ("rb_spectator_read_live", _I32, [_P, _P, _P]),
    ("rb_spectator_totals", _I32, [_P, _P]),
    ("rb_spectator_state_bytes", _I32, [_P]),
    ("rb_spectator_input_bytes", _I32, [_P]),
    ("rb_decode_input_packets", _I32, [_I32, _P, _I32, _I32, _I32, _I32, _I32, _P, ctypes.c_int64, _P, _P, _P, _I32,
                                        _P, _P]),
    ("rb_encode_input_packets", _I32, [_I32, _P, _I32, _I32, _I32, _I32, _P, _I32, _I32, _P, _P, _P, ctypes.c_int64,
                                        _P, _P]),
    ("rb_decode_input_packets_all", _I32, [_I32, _P, ctypes.c_uint32, _I32, _I32, _I32, _I32, _P, ctypes.c_int64, _P, _P,
                                            _P, _I32, _I32, _P, _P]),
    ("rb_encode_input_packets_all", _I32, [_I32, _P, ctypes.c_uint32, _I32, _I32, _I32, _P, _I32, _I32, _I32, _P, _P, _P,
                                            ctypes.c_int64, _P, _P]),
    ("rb_decode_input_packets_grouped", _I32, [_I32, _P, ctypes.c_uint32, _I32, _I32, _I32, _I32, _P, ctypes.c_int64, _P,
                                                _P, _P, _I32, _I32, _P, _P]),
    ("rb_encode_input_packets_grouped", _I32, [_I32, _P, ctypes.c_uint32, _I32, _I32, _I32, _P, _I32, _I32, _I32, _P, _P,
                                                _P, ctypes.c_int64, _P, _P]),
    ("rb_parse_datagrams_all", _I32, [_I32, _P, ctypes.c_uint32, _I32, _I32, ctypes.POINTER(RbDatagramParse)]),
    ("rb_build_datagrams_all", _I32, [_I32, _P, ctypes.c_uint32, _I32, _I32, ctypes.POINTER(RbDatagramBuild)]),
    ("rb_endpoint_protocol_poll_all", _I32, [_I32, _P, ctypes.c_uint32, _I32, _I32, ctypes.POINTER(RbEndpointProtocol)]),
]

# the entry points that return a 64-bit size
SIZE_SIGNATURES = [
    ("rb_p2p_session_record_bytes", ctypes.c_int64, [_P]),
    ("rb_spectator_session_record_bytes", ctypes.c_int64, [_P]),
]

_lib = None


def load() -> ctypes.CDLL:
    """Load the HIP engine library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make -C ggrs_amd/csrc` "
            "(or __graft_entry__.build()); the engine has no CPU fallback."
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, res, args in SIGNATURES + SIZE_SIGNATURES:
        if os.environ.get("GGRS_AMD_LIB") and not hasattr(lib, name):
            continue  # an older experiment build may lack newer entry points
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
