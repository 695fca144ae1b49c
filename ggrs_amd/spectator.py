"""SpectatorSession batches over the C ABI (include/ggrs_amd.h rb_spectator_*).

Mirrors sessions/p2p_spectator_session.rs for ``num_sessions`` independent
spectators, each a rollback-free replica of one host session: it advances only
on the inputs its host has confirmed (``P2PSession.export_confirmed_inputs``,
p2p_session.rs:676-703) and catches up when it falls behind.  The network
layer is the caller's, as for the P2P batches: per tick it hands over the
newest frame the host's Input messages have delivered and the inputs by frame.
Built by ``SessionBuilder.with_max_frames_behind(..).with_catchup_speed(..)
.start_spectator_session()`` (builder.rs:210-244, 310-334).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
from .migrate import _Movable
from .p2p import _dev_ptr
from .session import (DeviceError, InvalidRequest, Panic, PredictionThreshold, SpectatorTooFarBehind, _StreamOrdered,
                      input_dtype)


class SpectatorSession(_Movable, _StreamOrdered):
    """p2p_spectator_session.rs:22-254 for ``num_sessions`` sessions that start Running.

    Device work runs on the batch's own HIP stream (or the one set_stream
    chose), ordered against torch's current stream at every call
    (_StreamOrdered)."""

    _MOVE = "rb_spectator"  # export_sessions, import_sessions, import_refused, record_bytes (migrate.py)

    def __init__(self, lib, handle, game, cfg):
        self._lib = lib
        self._h = handle
        self.game = game
        self.num_sessions = int(cfg.num_sessions)
        self._num_players = int(cfg.num_players)
        self.max_frames_behind = int(cfg.max_frames_behind)
        self.catchup_speed = int(cfg.catchup_speed)
        self.state_bytes = lib.rb_spectator_state_bytes(handle)
        self.input_dtype = input_dtype(game, lib.rb_spectator_input_bytes(handle))
        self._device = int(cfg.device)
        self.delivery_ring = 0  # set_delivery_ring: R, or 0 for a linear host_inputs
        self._bind(self._device, lib.rb_spectator_get_stream(handle) or 0)

    def close(self):
        if self._h:
            self._lib.rb_spectator_destroy(self._h)  # synchronises the batch stream first
            self._h = None
            self._stream = None
            self._drain()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, st):
        if st != L.RB_OK:
            msg = (self._lib.rb_spectator_last_error(self._h) or b"").decode()
            if st == L.RB_INVALID_REQUEST:
                raise InvalidRequest(msg)
            raise DeviceError(msg) if st == L.RB_DEVICE_ERROR else Panic(msg)

    def num_players(self) -> int:  # :169-171
        return self._num_players

    def set_stream(self, stream) -> None:
        self._check(self._lib.rb_spectator_set_stream(self._h, ctypes.c_void_p(stream.cuda_stream if stream else 0)))
        self._bind(self._device, self._lib.rb_spectator_get_stream(self._h) or 0)

    def receive_host_status(self, last_frames, disconnected) -> None:
        """The host's connect status as its Input messages carry it (:243-245 over
        protocol.rs:629-636): last_frames [P, S] int32 and disconnected [P, S] uint8 CUDA
        tensors, what ``P2PSession.export_confirmed_inputs`` writes.  Merged: disconnected
        is OR-ed, last_frame takes the maximum."""
        import torch
        lp, lk = _dev_ptr(last_frames)
        dp, dk = _dev_ptr(disconnected)
        assert tuple(lk.shape) == (self._num_players, self.num_sessions) and tuple(dk.shape) == tuple(lk.shape)
        assert lk.dtype == torch.int32 and dk.dtype in (torch.uint8, torch.bool)
        cur = self._pre()
        st = self._lib.rb_spectator_receive_host_status(self._h, lp, dp)
        self._post(cur, (lk, dk))
        self._check(st)

    def restart_sessions(self, sessions=None) -> None:
        """start_spectator_session again in every session where `sessions` is true (None: all),
        between ticks (rb_spectator_restart_sessions): the spectator follows its host's next
        match from frame 0.  The other sessions are untouched; totals() continues since create."""
        m = None
        if sessions is not None:
            m = np.ascontiguousarray(np.broadcast_to(np.asarray(sessions), (self.num_sessions,)), dtype=np.uint8)
        st = self._lib.rb_spectator_restart_sessions(self._h, None if m is None else m.ctypes.data_as(ctypes.c_void_p))
        self._check(st)

    def set_delivery_ring(self, ring_frames: int) -> None:
        """host_inputs becomes a ring [R, P, S] indexed by each spectator's own frame, frame f in
        slot f & (R - 1) (rb_spectator_set_delivery_ring): what a host batch in ring mode
        exports.  R a power of two >= 128; 0 returns to the linear layout.  The ring's head may
        lead the host_upto a spectator is handed by at most R - 60 frames."""
        self._check(self._lib.rb_spectator_set_delivery_ring(self._h, int(ring_frames)))
        self.delivery_ring = int(ring_frames)

    def run_ticks(self, host_upto, host_inputs) -> None:
        """T ticks of advance_frame + handle_requests in one device launch.

        host_upto   [T, S] int32: the newest frame delivered before each tick (NULL_FRAME: none)
        host_inputs [F, P, S] Input values by frame, complete up to the largest host_upto
                    (after set_delivery_ring(R): the ring [R, P, S])
        Both torch CUDA tensors on the batch's device."""
        import torch
        T = int(host_upto.shape[0])
        assert tuple(host_upto.shape) == (T, self.num_sessions) and host_upto.dtype == torch.int32
        assert tuple(host_inputs.shape[1:]) == (self._num_players, self.num_sessions)
        assert not self.delivery_ring or int(host_inputs.shape[0]) == self.delivery_ring, \
            "the batch has a delivery ring: host_inputs holds exactly its R frames"
        assert host_inputs.element_size() == np.dtype(self.input_dtype).itemsize
        up, uk = _dev_ptr(host_upto)
        ip, ik = _dev_ptr(host_inputs)
        cur = self._pre()
        st = self._lib.rb_spectator_run_ticks(self._h, T, up, ip, int(host_inputs.shape[0]))
        self._post(cur, (uk, ik))
        self._check(st)

    def advance_frame(self, host_upto, host_inputs) -> np.ndarray:
        """One tick (:109-139): host_upto [S].  Returns the per-session rb_status [S]; raises
        PredictionThreshold / SpectatorTooFarBehind only when every session reports it
        (a batch of one behaves like the reference's session)."""
        self.run_ticks(host_upto[None], host_inputs)
        st, _ = self.status()
        if (st == L.RB_PREDICTION_THRESHOLD).all():
            raise PredictionThreshold("every session waits for its host's inputs")
        if (st == L.RB_SPECTATOR_TOO_FAR_BEHIND).all():
            raise SpectatorTooFarBehind("every session is more than 60 frames behind its host")
        return st

    def status(self):
        """(rb_status [S], AdvanceFrame count [S]) of the last tick (count -1 before the first)."""
        st = np.empty(self.num_sessions, np.int32)
        na = np.empty(self.num_sessions, np.int32)
        self._check(self._lib.rb_spectator_read_status(self._h, st.ctypes.data_as(ctypes.c_void_p),
                                                       na.ctypes.data_as(ctypes.c_void_p)))
        return st, na

    def frames(self):
        """(current_frame [S], last_recv_frame [S]); both NULL_FRAME at first (:67-68)."""
        c = np.empty(self.num_sessions, np.int32)
        r = np.empty(self.num_sessions, np.int32)
        self._check(self._lib.rb_spectator_read_frames(self._h, c.ctypes.data_as(ctypes.c_void_p),
                                                       r.ctypes.data_as(ctypes.c_void_p)))
        return c, r

    def frames_behind_host(self) -> np.ndarray:  # :80-84
        c, r = self.frames()
        return r - c

    def read_live(self):
        """(images [S, state_bytes], checksums [S, 2] u64 lo/hi): the state after
        current_frame (frame word current_frame + 1) and the checksum the host's cell of
        that frame holds (computed by every launch)."""
        img = np.zeros((self.num_sessions, self.state_bytes), np.uint8)
        cs = np.zeros((self.num_sessions, 2), np.uint64)
        self._check(self._lib.rb_spectator_read_live(self._h, img.ctypes.data_as(ctypes.c_void_p),
                                                     cs.ctypes.data_as(ctypes.c_void_p)))
        return img, cs

    def totals(self):
        """Since create: (AdvanceFrames, PredictionThreshold ticks, SpectatorTooFarBehind ticks)."""
        c = (ctypes.c_uint64 * 3)()
        self._check(self._lib.rb_spectator_totals(self._h, c))
        return tuple(int(x) for x in c)
