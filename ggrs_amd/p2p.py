"""P2PSession batches over the C ABI (include/ggrs_amd.h rb_p2p_*).

Mirrors sessions/p2p_session.rs for ``num_sessions`` independent sessions seen
from one peer.  The network layer is the caller's: per tick it hands over, for
every remote handle, the newest delivered frame and the inputs by frame — what
UdpProtocol's Event::Input stream (p2p_session.rs:838-852) carries.  Built by
``SessionBuilder.add_player(...).start_p2p_session()`` (builder.rs:251-308).

``synth_network`` produces a deterministic synthetic delivery schedule (per
session latency + jitter) for tests and the bench.
"""
from __future__ import annotations

import ctypes
import enum

import numpy as np

from . import _lib as L
from .migrate import _Movable
from .session import DeviceError, InvalidRequest, Panic, _StreamOrdered, input_dtype
from .synth import SEED, splitmix64


class PlayerType(enum.Enum):  # lib.rs:115-124 (spectators are batches of their own: ggrs_amd.spectator)
    Local = "local"
    Remote = "remote"


def _dev_ptr(x):
    """(pointer, keepalive) of a torch CUDA tensor."""
    import torch
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise TypeError("P2P tensors must be torch CUDA tensors (device memory, stream ordered)")
    x = x.contiguous()
    return ctypes.c_void_p(x.data_ptr()), x


class P2PSession(_Movable, _StreamOrdered):
    """p2p_session.rs:116-929 (rollback path) for ``num_sessions`` sessions.

    Device work runs on the batch's own HIP stream (or the one set_stream
    chose) and is ordered against torch's current stream at every call
    (_StreamOrdered): inputs made on torch's stream are complete before a
    launch reads them, and tensors a call writes (checksum reports) are
    complete before later torch work on the current stream reads them."""

    _MOVE = "rb_p2p"  # export_sessions, import_sessions, import_refused, record_bytes (migrate.py)

    def __init__(self, lib, handle, game, cfg):
        self._lib = lib
        self._h = handle
        self.game = game
        self.num_sessions = int(cfg.num_sessions)
        self.num_players = int(cfg.num_players)
        self.max_prediction = int(cfg.max_prediction)
        self.input_delay = int(cfg.input_delay)
        self.remote_delay = int(cfg.remote_delay)
        self.sparse_saving = bool(cfg.sparse_saving)
        self.local_mask = int(cfg.local_mask)
        self.desync_interval = int(cfg.desync_interval)
        self.state_bytes = lib.rb_p2p_state_bytes(handle)
        self.input_dtype = input_dtype(game, lib.rb_p2p_input_bytes(handle))
        self._device = int(cfg.device)
        self.delivery_ring = 0  # set_delivery_ring: R, or 0 for linear by-frame tensors
        self._bind(self._device, lib.rb_p2p_get_stream(handle) or 0)

    def close(self):
        if self._h:
            self._lib.rb_p2p_destroy(self._h)  # synchronises the batch stream first
            self._h = None
            self._stream = None
            self._drain()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != L.RB_OK:
            msg = (self._lib.rb_p2p_last_error(self._h) or b"").decode()
            if st == L.RB_INVALID_REQUEST:
                raise InvalidRequest(msg)
            raise DeviceError(msg) if st == L.RB_DEVICE_ERROR else Panic(msg)

    def local_player_handles(self):  # p2p_session.rs:416-419
        return [h for h in range(self.num_players) if (self.local_mask >> h) & 1]

    def remote_player_handles(self):  # :421-424
        return [h for h in range(self.num_players) if not (self.local_mask >> h) & 1]

    def set_stream(self, stream) -> None:
        self._check(self._lib.rb_p2p_set_stream(self._h, ctypes.c_void_p(stream.cuda_stream if stream else 0)))
        self._bind(self._device, self._lib.rb_p2p_get_stream(self._h) or 0)

    def fanout_state(self):
        """The adaptive fan-out (rb_p2p_fanout_state): (active, select fraction of the last
        measured window or -1, windows measured, times turned off)."""
        a, w, o = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        f = ctypes.c_double()
        self._check(self._lib.rb_p2p_fanout_state(self._h, ctypes.byref(a), ctypes.byref(f), ctypes.byref(w),
                                                  ctypes.byref(o)))
        return bool(a.value), f.value, w.value, o.value

    def run_ticks(self, local_inputs, remote_upto, remote_inputs, run_mask=None) -> None:
        """T ticks: [poll_remote_clients, add_local_input for every local handle,
        advance_frame, handle_requests] x T in one device launch.

        local_inputs  [T, P, S] Input values (remote handles' rows ignored)
        remote_upto   [T, P, S] int32 newest delivered frame per remote handle
        remote_inputs [F, P, S] Input values by frame (local handles' rows ignored); after
                      set_delivery_ring(R) the ring [R, P, S], frame f of a session in slot f & (R - 1)
        run_mask      None, or [T, S] uint8: 0 parks session s in tick t, which then only
                      polls (rb_p2p_run_ticks_paced; T one-tick sequences on the stream)
        All torch CUDA tensors on the batch's device."""
        import torch
        T = int(local_inputs.shape[0])
        assert tuple(local_inputs.shape[1:]) == (self.num_players, self.num_sessions)
        assert tuple(remote_upto.shape) == (T, self.num_players, self.num_sessions)
        assert tuple(remote_inputs.shape[1:]) == (self.num_players, self.num_sessions)
        assert not self.delivery_ring or int(remote_inputs.shape[0]) == self.delivery_ring, \
            "the batch has a delivery ring: remote_inputs holds exactly its R frames"
        lp, lk = _dev_ptr(local_inputs)
        up, uk = _dev_ptr(remote_upto)
        rp, rk = _dev_ptr(remote_inputs)
        keep = (lk, uk, rk)
        if run_mask is not None:
            assert run_mask.dtype == torch.uint8 and tuple(run_mask.shape) == (T, self.num_sessions)
            mp, mk = _dev_ptr(run_mask)
            keep += (mk,)
        cur = self._pre()
        stride = self.num_players * self.num_sessions * lk.element_size()
        if run_mask is None:
            st = self._lib.rb_p2p_run_ticks(self._h, T, lp, stride, up, rp, int(remote_inputs.shape[0]))
        else:
            st = self._lib.rb_p2p_run_ticks_paced(self._h, T, lp, stride, up, rp, int(remote_inputs.shape[0]), mp)
        self._post(cur, keep)
        self._check(st)

    def run_ticks_packets(self, local_inputs, packets, lengths, start_frames, decode_status=None, acks=None) -> None:
        """T ticks fed by the peers' input packets (rb_p2p_run_ticks_packets):
        each tick decodes every remote endpoint's packet inside its poll
        (UdpProtocol::on_input), then runs as run_ticks.

        local_inputs  [T, P, S] Input values (remote handles' rows ignored)
        packets       [T, P, S, stride] uint8 (stride a multiple of 16, >= 32)
        lengths, start_frames [T, P, S] int32 (length 0: no packet)
        decode_status, acks   None or [P, S] int32 outputs: the last tick's decode
                      result per endpoint, the newest frame received per endpoint"""
        import torch
        T = int(local_inputs.shape[0])
        assert tuple(local_inputs.shape[1:]) == (self.num_players, self.num_sessions)
        assert tuple(packets.shape[:3]) == (T, self.num_players, self.num_sessions) and packets.dim() == 4
        assert tuple(lengths.shape) == tuple(start_frames.shape) == (T, self.num_players, self.num_sessions)
        # the kernel reads packets as bytes and lengths / start frames as int32, and writes int32 outputs
        assert packets.dtype == torch.uint8, "packets must be uint8 (the row stride is a byte count)"
        assert lengths.dtype == start_frames.dtype == torch.int32, "lengths and start_frames must be int32"
        for o in (decode_status, acks):
            assert o is None or o.dtype == torch.int32, "decode_status / acks must be int32"
        lp, lk = _dev_ptr(local_inputs)
        pp, pk = _dev_ptr(packets)
        np_, nk = _dev_ptr(lengths)
        sp, sk = _dev_ptr(start_frames)
        keep = [lk, pk, nk, sk]
        outs = []
        for o in (decode_status, acks):
            if o is None:
                outs.append(None)
            else:
                assert tuple(o.shape) == (self.num_players, self.num_sessions) and o.is_contiguous()
                op, ok = _dev_ptr(o)
                outs.append(op)
                keep.append(ok)
        cur = self._pre()
        stride = self.num_players * self.num_sessions * lk.element_size()
        self._check(self._lib.rb_p2p_run_ticks_packets(self._h, T, lp, stride, pp, int(packets.shape[3]), np_, sp,
                                                       outs[0], outs[1]))
        self._post(cur, tuple(keep), outputs=decode_status is not None or acks is not None)

    def disconnect_player(self, handle: int, sessions=None) -> None:
        """P2PSession::disconnect_player(handle) (p2p_session.rs:430-456) in every
        session where `sessions` is true (None: all), between ticks.  Raises
        InvalidRequest like the reference (invalid handle, local player, already
        disconnected) and then applies nothing."""
        m = None
        if sessions is not None:
            m = np.ascontiguousarray(np.broadcast_to(np.asarray(sessions), (self.num_sessions,)), dtype=np.uint8)
        st = self._lib.rb_p2p_disconnect_player(self._h, int(handle),
                                               None if m is None else m.ctypes.data_as(ctypes.c_void_p))
        if st == L.RB_INVALID_REQUEST:
            raise InvalidRequest((self._lib.rb_p2p_last_error(self._h) or b"").decode())
        self._check(st)

    def restart_sessions(self, sessions=None) -> None:
        """Drop the P2PSession and start_p2p_session again (builder.rs:251-308) in every session
        where `sessions` is true (None: all), between ticks (rb_p2p_restart_sessions): the
        session is what a freshly created batch holds, its next tick is its frame 0 and its
        deliveries, packets and export rows count from 0 again.  The other sessions are untouched;
        counters() and totals() continue since create.  Read a session's desync events, wait
        recommendations, network events or parked ticks before restarting it."""
        m = None
        if sessions is not None:
            m = np.ascontiguousarray(np.broadcast_to(np.asarray(sessions), (self.num_sessions,)), dtype=np.uint8)
        st = self._lib.rb_p2p_restart_sessions(self._h, None if m is None else m.ctypes.data_as(ctypes.c_void_p))
        if st == L.RB_INVALID_REQUEST:
            raise InvalidRequest((self._lib.rb_p2p_last_error(self._h) or b"").decode())
        self._check(st)

    def advance_frame(self, local_inputs, remote_upto, remote_inputs, run=None) -> None:
        """One tick (run_ticks with T = 1): local_inputs [P, S], remote_upto [P, S];
        run None, or [S] uint8: 0 parks the session for this tick."""
        self.run_ticks(local_inputs[None], remote_upto[None], remote_inputs, None if run is None else run[None])

    # -- pacing (ex_game_p2p.rs:80-122)
    def pace(self, out=None):
        """The next tick's run mask from frames_ahead (rb_p2p_pace): a uint8 CUDA tensor [S],
        stream ordered, no host copy.  A session that is ahead runs 10 ticks of every 11.
        Needs enable_time_sync; `out` may be reused."""
        import torch
        if out is None:
            out = torch.empty((self.num_sessions,), dtype=torch.uint8, device=f"cuda:{self._device}")
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.uint8 and tuple(out.shape) == (self.num_sessions,)
        cur = self._pre()
        st = self._lib.rb_p2p_pace(self._h, ctypes.c_void_p(out.data_ptr()))
        self._post(cur, (out,), outputs=True)
        self._check(st)
        return out

    def parked_ticks(self):
        """Ticks each session sat out since create, uint32 [S] (rb_p2p_read_pacing)."""
        out = np.empty(self.num_sessions, np.uint32)
        self._check(self._lib.rb_p2p_read_pacing(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def status(self):
        """(rb_status [S], LoadGameState frame [S] (NULL_FRAME = no rollback),
        AdvanceFrame count [S], SaveGameState count [S]) of the last tick."""
        st, lf, na, ns = (np.empty(self.num_sessions, np.int32) for _ in range(4))
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(self._lib.rb_p2p_read_status(self._h, p(st), p(lf), p(na), p(ns)))
        return st, lf, na, ns

    def frames(self):
        """(current_frame [S], last confirmed frame [S])."""
        c = np.empty(self.num_sessions, np.int32)
        k = np.empty(self.num_sessions, np.int32)
        self._check(self._lib.rb_p2p_read_frames(self._h, c.ctypes.data_as(ctypes.c_void_p),
                                                 k.ctypes.data_as(ctypes.c_void_p)))
        return c, k

    def read_queues(self):
        """InputQueue / ConnectionStatus bookkeeping [S, P, 8]: last_added_frame, inputs[tail].frame,
        length, last_requested_frame, prediction.frame, first_incorrect_frame, connect-status
        last_frame, disconnected (input_queue.rs:12-34, messages.rs:5-18)."""
        out = np.empty((self.num_sessions, self.num_players, 8), np.int32)
        self._check(self._lib.rb_p2p_read_queues(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def read_cells(self):
        """(frame tags [W, S], images [W, S, B], checksums [W, S, 2])."""
        W, S = self.max_prediction, self.num_sessions
        tags = np.empty((W, S), np.int32)
        img = np.zeros((W, S, self.state_bytes), np.uint8)
        cs = np.zeros((W, S, 2), np.uint64)
        self._check(self._lib.rb_p2p_read_cells(self._h, tags.ctypes.data_as(ctypes.c_void_p),
                                                img.ctypes.data_as(ctypes.c_void_p), cs.ctypes.data_as(ctypes.c_void_p)))
        return tags, img, cs

    def read_live(self):
        img = np.zeros((self.num_sessions, self.state_bytes), np.uint8)
        self._check(self._lib.rb_p2p_read_live(self._h, img.ctypes.data_as(ctypes.c_void_p)))
        return img

    def counters(self):
        """(PredictionThreshold hits, unexpected math paths, panicked sessions) since create."""
        c = (ctypes.c_uint32 * 3)()
        self._check(self._lib.rb_p2p_counters(self._h, c))
        return tuple(c)

    def totals(self):
        """Work executed since create: (AdvanceFrames, SaveGameStates, LoadGameStates,
        speculative selects, branch frames presimulated)."""
        c = (ctypes.c_uint64 * 5)()
        self._check(self._lib.rb_p2p_totals(self._h, c))
        return tuple(int(x) for x in c)

    # -- desync detection (p2p_session.rs:873-928)
    def take_checksum_reports(self, out=None):
        """The ChecksumReports every session sent since the last call, oldest
        first, as a CUDA int64 tensor [RB_P2P_REPORTS_PER_TAKE, S, 3] (one
        rb_checksum_report per row: checksum lo, hi, frame | mismatch << 32;
        frame NULL_FRAME = none).  Ordered against torch's current stream
        (_StreamOrdered): later work on it sees the reports; `out` may be reused."""
        import torch
        from .shard import REPORT_WORDS
        K = L.RB_P2P_REPORTS_PER_TAKE
        if out is None:
            out = torch.empty((K, self.num_sessions, REPORT_WORDS), dtype=torch.int64, device="cuda")
        assert out.is_cuda and out.is_contiguous() and tuple(out.shape) == (K, self.num_sessions, REPORT_WORDS)
        cur = self._pre()
        self._check(self._lib.rb_p2p_take_checksum_reports(self._h, ctypes.c_void_p(out.data_ptr())))
        self._post(cur, (out,), outputs=True)
        return out

    def receive_checksum_reports(self, handle: int, reports) -> None:
        """The peer behind remote `handle` sent `reports` ([K, S, 3] int64 CUDA
        tensor, take_checksum_reports layout): UdpProtocol::on_checksum_report."""
        r, keep = _dev_ptr(reports)
        assert keep.dim() == 3 and keep.shape[1] == self.num_sessions
        cur = self._pre()
        st = self._lib.rb_p2p_receive_checksum_reports(self._h, int(handle), r, int(keep.shape[0]))
        self._post(cur, (keep,))
        if st == L.RB_INVALID_REQUEST:
            raise InvalidRequest((self._lib.rb_p2p_last_error(self._h) or b"").decode())
        self._check(st)

    def desync_events(self):
        """(counts [S], frames [S, E], handles [S, E], local [S, E], remote [S, E]):
        GGRSEvent::DesyncDetected per session since create, the newest E in order."""
        E = L.RB_P2P_EVENTS_KEPT
        n = np.empty(self.num_sessions, np.uint32)
        fr = np.empty((self.num_sessions, E), np.int32)
        hd = np.empty((self.num_sessions, E), np.int32)
        lo = np.empty((self.num_sessions, E), np.uint64)
        ro = np.empty((self.num_sessions, E), np.uint64)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(self._lib.rb_p2p_read_desync_events(self._h, p(n), p(fr), p(hd), p(lo), p(ro)))
        return n, fr, hd, lo, ro

    def receive_peer_connect_status(self, endpoint: int, last_frames, disconnected) -> None:
        """The peer behind remote handle `endpoint` reports every player's ConnectionStatus
        (UdpProtocol::on_input, protocol.rs:627-636): last_frames [P, S] int32 and
        disconnected [P, S] uint8, CUDA tensors.  Needs with_peer_connect_status(True)."""
        lp, lk = _dev_ptr(last_frames)
        dp, dk = _dev_ptr(disconnected)
        assert tuple(lk.shape) == (self.num_players, self.num_sessions) and tuple(dk.shape) == tuple(lk.shape)
        cur = self._pre()
        st = self._lib.rb_p2p_receive_peer_connect_status(self._h, int(endpoint), lp, dp)
        self._post(cur, (lk, dk))
        if st == L.RB_INVALID_REQUEST:
            raise InvalidRequest((self._lib.rb_p2p_last_error(self._h) or b"").decode())
        self._check(st)

    # -- the spectators' feed (p2p_session.rs:303, 676-703)
    def export_confirmed_inputs(self, inputs_by_frame, upto, last_frames, disconnected) -> None:
        """send_confirmed_inputs_to_spectators for every session, between run_ticks calls:
        every frame up to the minimum last_frame of the connected players that was not
        exported before is written to inputs_by_frame [F, P, S] (Input values, absolute
        frames, all players; zero for a disconnected player past its last frame), then
        upto [S] int32 (newest frame exported so far, NULL_FRAME: none), last_frames [P, S]
        int32 and disconnected [P, S] uint8 (the host's connect status).  CUDA tensors,
        written in place; what SpectatorSession.run_ticks / receive_host_status read."""
        import torch
        P, S = self.num_players, self.num_sessions
        assert tuple(inputs_by_frame.shape[1:]) == (P, S) and inputs_by_frame.is_contiguous()
        assert inputs_by_frame.element_size() == np.dtype(self.input_dtype).itemsize
        assert not self.delivery_ring or int(inputs_by_frame.shape[0]) == self.delivery_ring
        assert tuple(upto.shape) == (S,) and upto.dtype == torch.int32 and upto.is_contiguous()
        assert tuple(last_frames.shape) == (P, S) and last_frames.dtype == torch.int32 and last_frames.is_contiguous()
        assert tuple(disconnected.shape) == (P, S) and disconnected.dtype == torch.uint8 and disconnected.is_contiguous()
        ptrs = [_dev_ptr(x)[0] for x in (inputs_by_frame, upto, last_frames, disconnected)]
        cur = self._pre()
        st = self._lib.rb_p2p_export_confirmed_inputs(self._h, ptrs[0], int(inputs_by_frame.shape[0]), ptrs[1], ptrs[2],
                                                      ptrs[3])
        self._post(cur, (inputs_by_frame, upto, last_frames, disconnected), outputs=True)
        self._check(st)

    # -- per-session delivery rings
    def set_delivery_ring(self, ring_frames: int) -> None:
        """Every by-frame tensor of the batch (run_ticks' remote_inputs, the inputs_by_frame of
        export_confirmed_inputs and export_local_inputs) becomes a ring [R, P, S] indexed by each
        session's own frame, frame f in slot f & (R - 1) (rb_p2p_set_delivery_ring): sessions of
        one batch may then sit any number of frames apart.  R a power of two >= 128; 0 returns to
        the linear layout.  Between run_ticks calls; no device work.  The caller keeps every frame
        between a session's last delivered frame and the call's largest watermark in its slot
        (``DeliveryRing``); older content of a slot is never read."""
        self._check(self._lib.rb_p2p_set_delivery_ring(self._h, int(ring_frames)))
        self.delivery_ring = int(ring_frames)

    def export_local_inputs(self, inputs_by_frame, sent) -> None:
        """UdpProtocol::send_input in tensor form (rb_p2p_export_local_inputs), between run_ticks
        calls: for every local handle h the inputs of frames sent[h, s] + 1 .. the newest frame
        add_local_input queued go to inputs_by_frame [F, P, S] (the batch's layout: linear, or the
        delivery ring), and sent [P, S] int32 becomes the last frame written.  Remote handles'
        rows of both tensors are untouched.  sent is the caller's: NULL_FRAME at first and after
        restarting a session.  At most the newest 128 frames are still there; older ones are
        skipped.  A peer batch reads the same tensor as its remote_inputs, with (an older copy
        of) sent as its remote_upto."""
        import torch
        P, S = self.num_players, self.num_sessions
        assert tuple(inputs_by_frame.shape[1:]) == (P, S) and inputs_by_frame.is_cuda and inputs_by_frame.is_contiguous()
        assert inputs_by_frame.element_size() == np.dtype(self.input_dtype).itemsize
        assert not self.delivery_ring or int(inputs_by_frame.shape[0]) == self.delivery_ring
        assert tuple(sent.shape) == (P, S) and sent.dtype == torch.int32 and sent.is_cuda and sent.is_contiguous()
        cur = self._pre()
        st = self._lib.rb_p2p_export_local_inputs(self._h, ctypes.c_void_p(inputs_by_frame.data_ptr()),
                                                  int(inputs_by_frame.shape[0]), ctypes.c_void_p(sent.data_ptr()))
        self._post(cur, (inputs_by_frame, sent), outputs=True)
        self._check(st)

    def export_status(self):
        """(status [S]: RB_P2P_EXPORT_OK, or RB_P2P_EXPORT_OVERRUN for a session whose input
        ring overwrote frames it still had to export (it exports nothing more);
        next_spectator_frame [S])."""
        st = np.empty(self.num_sessions, np.int32)
        nx = np.empty(self.num_sessions, np.int32)
        self._check(self._lib.rb_p2p_read_export_status(self._h, st.ctypes.data_as(ctypes.c_void_p),
                                                        nx.ctypes.data_as(ctypes.c_void_p)))
        return st, nx

    # -- time sync (time_sync.rs; p2p_session.rs:551, 745-776; protocol.rs:268-300, 697-708)
    def enable_time_sync(self, fps: int = 60) -> None:
        """SessionBuilder::with_fps (builder.rs:186-199; DEFAULT_FPS 60) and the batch's time
        sync on: from now on every run_ticks call also updates frames_ahead, the
        per-endpoint advantages and the WaitRecommendation events.  Before the first tick, once."""
        self._check(self._lib.rb_p2p_time_sync_enable(self._h, int(fps)))

    def receive_quality(self, handle: int, rtt_ms=None, frame_advantage=None) -> None:
        """The peer behind remote `handle` answered a QualityReport (rtt_ms: round trip in
        milliseconds) or sent one (frame_advantage, an i8 on the wire): int32 CUDA tensors [S],
        None leaves the value as it is.  Between run_ticks calls."""
        import torch
        ptrs, keep = [], []
        for x in (rtt_ms, frame_advantage):
            if x is None:
                ptrs.append(None)
                continue
            p, k = _dev_ptr(x)
            assert k.dtype == torch.int32 and tuple(k.shape) == (self.num_sessions,)
            ptrs.append(p)
            keep.append(k)
        cur = self._pre()
        st = self._lib.rb_p2p_receive_quality(self._h, int(handle), ptrs[0], ptrs[1])
        self._post(cur, tuple(keep))
        self._check(st)

    def _time_sync(self):
        S, P = self.num_sessions, self.num_players
        fa = np.empty(S, np.int32)
        la, ra, rtt = (np.empty((P, S), np.int32) for _ in range(3))
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(self._lib.rb_p2p_read_time_sync(self._h, p(fa), p(la), p(ra), p(rtt)))
        return fa, la, ra, rtt

    def frames_ahead(self):
        """P2PSession::frames_ahead (p2p_session.rs:551) per session, int32 [S]."""
        return self._time_sync()[0]

    def read_time_sync(self):
        """(frames_ahead [S], local_frame_advantage [P, S], remote_frame_advantage [P, S], rtt_ms [P, S])."""
        return self._time_sync()

    def network_stats(self, handle: int):
        """The NetworkStats fields this path owns (protocol.rs:294-300) for remote `handle`, each
        int32 [S]: ping (ms), local_frames_behind, remote_frames_behind.  send_queue_len and
        kbps_sent are the network layer's."""
        if not 0 <= int(handle) < self.num_players or (self.local_mask >> int(handle)) & 1:  # p2p_session.rs:469-484
            raise InvalidRequest("Given player handle not referring to a remote player or spectator")
        _, la, ra, rtt = self._time_sync()
        return {"ping": rtt[handle], "local_frames_behind": la[handle], "remote_frames_behind": ra[handle]}

    def wait_recommendations(self):
        """(counts [S], frames [S, E], skip_frames [S, E]): GGRSEvent::WaitRecommendation per
        session since enable_time_sync, the newest E = RB_P2P_WAIT_EVENTS_KEPT in order with the
        current_frame they were raised at (frame NULL_FRAME: none)."""
        E = L.RB_P2P_WAIT_EVENTS_KEPT
        n = np.empty(self.num_sessions, np.uint32)
        fr = np.empty((self.num_sessions, E), np.int32)
        sk = np.empty((self.num_sessions, E), np.int32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(self._lib.rb_p2p_read_wait_recommendations(self._h, p(n), p(fr), p(sk)))
        return n, fr, sk

    def export_time_sync(self, frames_ahead=None, local_adv=None) -> None:
        """frames_ahead [S] and local_frame_advantage [P, S] (the QualityReport payload per
        endpoint) into int32 CUDA tensors, stream ordered, no synchronisation."""
        import torch
        S, P = self.num_sessions, self.num_players
        ptrs, keep = [], []
        for x, shape in ((frames_ahead, (S,)), (local_adv, (P, S))):
            if x is None:
                ptrs.append(None)
                continue
            assert x.is_cuda and x.is_contiguous() and x.dtype == torch.int32 and tuple(x.shape) == shape
            ptrs.append(ctypes.c_void_p(x.data_ptr()))
            keep.append(x)
        cur = self._pre()
        st = self._lib.rb_p2p_export_time_sync(self._h, ptrs[0], ptrs[1])
        self._post(cur, tuple(keep), outputs=True)
        self._check(st)

    # -- endpoint liveness (protocol.rs:377-394, 555-562, 621-626; p2p_session.rs:818-847)
    def enable_liveness(self, disconnect_timeout_ms: int = 2000, notify_start_ms: int = 500) -> None:
        """SessionBuilder::with_disconnect_timeout / with_disconnect_notify_delay (builder.rs:175-184)
        and the batch's receive timers on (rb_p2p_liveness_enable).  Once, before or after the
        first tick; needs 0 <= notify_start_ms <= disconnect_timeout_ms."""
        self._check(self._lib.rb_p2p_liveness_enable(self._h, int(disconnect_timeout_ms), int(notify_start_ms)))

    def poll_liveness(self, now_ms: int, received, disconnect_requested=None, state_out=None) -> None:
        """The timer half of poll_remote_clients for every session at the caller's clock `now_ms`
        (rb_p2p_poll_liveness): one launch, stream ordered, no host copy.  uint8 CUDA tensors [P, S]:
        received (a message of any kind came from that endpoint since the last poll),
        disconnect_requested (None, or the flag of the peer's Input message) and state_out (None, or
        written: bit 0 notify sent, bit 1 disconnect event sent, bit 2 player disconnected).  A silent
        peer raises NetworkInterrupted, then Disconnected, and is disconnected as by
        disconnect_player; between run_ticks calls."""
        import torch
        shape = (self.num_players, self.num_sessions)
        ptrs, keep = [], []
        for x in (received, disconnect_requested, state_out):
            if x is None:
                ptrs.append(None)
                continue
            assert x.is_cuda and x.is_contiguous() and x.dtype == torch.uint8 and tuple(x.shape) == shape
            ptrs.append(ctypes.c_void_p(x.data_ptr()))
            keep.append(x)
        assert received is not None
        cur = self._pre()
        st = self._lib.rb_p2p_poll_liveness(self._h, int(now_ms), ptrs[0], ptrs[1], ptrs[2])
        self._post(cur, tuple(keep), outputs=state_out is not None)
        self._check(st)

    def network_events(self):
        """(counts [S], kinds [S, E], handles [S, E], values [S, E]): GGRSEvent::NetworkInterrupted
        (RB_NET_INTERRUPTED, value = disconnect_timeout in ms), NetworkResumed and Disconnected per
        session since enable_liveness or its restart, the newest E = RB_P2P_NET_EVENTS_KEPT in order
        (kind 0, handle -1: none)."""
        E = L.RB_P2P_NET_EVENTS_KEPT
        n = np.empty(self.num_sessions, np.uint32)
        kd, hd, vl = (np.empty((self.num_sessions, E), np.int32) for _ in range(3))
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(self._lib.rb_p2p_read_network_events(self._h, p(n), p(kd), p(hd), p(vl)))
        return n, kd, hd, vl

    def read_liveness(self):
        """(last_recv_ms int64 [P, S], state uint8 [P, S]): every endpoint's last receive time on the
        caller's clock (-1: no poll yet, and local handles) and poll_liveness's state_out bits."""
        st = np.empty((self.num_players, self.num_sessions), np.int64)
        fl = np.empty((self.num_players, self.num_sessions), np.uint8)
        self._check(self._lib.rb_p2p_read_liveness(self._h, st.ctypes.data_as(ctypes.c_void_p),
                                                   fl.ctypes.data_as(ctypes.c_void_p)))
        return st, fl

    def debug_time_sync_windows(self):
        """The TimeSync windows, int32 [2 (local, remote), 30, P, S] (tests)."""
        out = np.empty((2, 30, self.num_players, self.num_sessions), np.int32)
        self._check(self._lib.rb_p2p_debug_read_time_sync_windows(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def debug_corrupt(self, session: int, word: int, xor_mask: int) -> None:
        """Flip canonical state word `word` of the live state and every cell of `session`."""
        st = self._lib.rb_p2p_debug_corrupt(self._h, int(session), int(word), ctypes.c_uint32(xor_mask & 0xFFFFFFFF))
        if st == L.RB_INVALID_REQUEST:
            raise InvalidRequest((self._lib.rb_p2p_last_error(self._h) or b"").decode())
        self._check(st)

    def profile_enable(self, on: bool) -> None:
        self._check(self._lib.rb_p2p_profile_enable(self._h, int(on)))

    def profile_take(self):
        ms = ctypes.c_double()
        n = ctypes.c_int32()
        self._check(self._lib.rb_p2p_profile_take(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def launch_clock_arm(self, launches: int) -> None:
        """The kernel's own clock for the next ``launches`` launches (rb_p2p_launch_clock_arm)."""
        self._check(self._lib.rb_p2p_launch_clock_arm(self._h, int(launches)))

    def launch_clock_read(self, cap: int):
        """Per launch since the arm: microseconds from its first wave's start to its last wave's end."""
        out = (ctypes.c_uint64 * (2 * cap))()
        n = ctypes.c_int32()
        self._check(self._lib.rb_p2p_launch_clock_read(self._h, out, int(cap), ctypes.byref(n)))
        return [(out[2 * i + 1] - out[2 * i]) / 100.0 for i in range(n.value)]


def synth_network(num_sessions: int, num_players: int, ticks: int, local_mask: int, remote_delay: int,
                  min_lag: int = 1, max_lag: int = 4, seed: int = SEED, first_session: int = 0,
                  dtype=np.uint8, mask: int = 0x0F):
    """A deterministic two-way network of peers in lock-step (numpy).

    Remote handle h's peer adds its local input for its frame f at frame
    f + remote_delay and sends it; it reaches us ``lag`` ticks later, with lag
    drawn per (session, tick) in [min_lag, max_lag] by splitmix64.  Deliveries
    are in order (UdpProtocol's sequencing): remote_upto[t] is the running
    maximum of (t - 1 - lag + remote_delay).

    Returns (local_inputs [T, P, S], remote_upto int32 [T, P, S],
    remote_inputs [T + remote_delay, P, S] by frame)."""
    from .synth import synth_inputs
    S, P, T = num_sessions, num_players, ticks
    inputs = synth_inputs(S, P, T, seed=seed, mask=mask, dtype=dtype, first_session=first_session)
    remote_in = np.zeros((T + remote_delay, P, S), dtype)
    remote_in[remote_delay:] = inputs  # the peer's input for its frame f lands at frame f + delay
    s = np.arange(first_session, first_session + S, dtype=np.uint64)[None, :]
    p = np.arange(P, dtype=np.uint64)[:, None]
    upto = np.empty((T, P, S), np.int32)
    run = np.full((P, S), -1, np.int64)
    span = max_lag - min_lag + 1
    for t in range(T):
        h = splitmix64(np.uint64(seed ^ 0x6E6574) ^ ((s << np.uint64(24)) + (p << np.uint64(20)) + np.uint64(t)))
        lag = min_lag + (h % np.uint64(span)).astype(np.int64)
        run = np.maximum(run, t - 1 - lag + remote_delay)
        upto[t] = np.minimum(run, T + remote_delay - 1)
    for hnd in range(P):
        if (local_mask >> hnd) & 1:
            upto[:, hnd] = -1
    return inputs, upto, remote_in
