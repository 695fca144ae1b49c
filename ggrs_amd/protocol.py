"""UdpProtocol's handshake, state machine and send timers over tensors (include/ggrs_amd.h
rb_endpoint_protocol_poll_all): which message every endpoint of a batch
owes this poll, and when, decided in one launch.

The endpoint of handle h, session s owns row (h, s) of every [P, S] tensor, as in ggrs_amd.datagram;
rows of handles outside handle_mask are untouched.  EndpointProtocol owns the state and the output
tensors as DeliveryRing owns its ring; a fresh endpoint is all zero bytes.  poll() runs on the
current torch stream and does not synchronise; a refused request raises InvalidRequest before
anything runs.
"""
from __future__ import annotations

import ctypes

from . import _lib as L
from .datagram import REPORT_WORDS, _opt, _rows, _shape
from .wire import _call, _ptr

NUM_SYNC_PACKETS = 5  # network/mod.rs
UDP_HEADER_SIZE = 28  # network/mod.rs: what network_stats adds per packet
STATE_TENSORS = ("ep_state", "sync_remaining", "sync_nonces", "sync_valid", "sync_next", "stamps", "packets_sent",
                 "last_newest", "remote_magic")
STAMPS = ("last_send", "last_input_recv", "last_quality_report", "shutdown_at", "stats_start")


class EndpointProtocol:
    """The protocol state of P x S endpoints and what one poll decided for them.

    State (in/out; the last axis is the session, so a session is a column of every tensor):
      ep_state uint8 [P, S] (RB_EP_*), sync_remaining int32 [P, S], sync_nonces int32 [8, P, S] (the
      u32 bits), sync_valid / sync_next uint8 [P, S], stamps int64 [5, P, S] (STAMPS), packets_sent
      int64 [P, S], last_newest int32 [P, S], remote_magic int16 [P, S] -> parse_datagrams
    Outputs of the last poll:
      input_lengths int32 [P, S] -> build_datagrams' lengths
      ack_due, reply_due, report_due, keepalive_due uint8 [P, S] -> build_datagrams' ack_owed,
          reply_owed, report_due, keepalive_due
      sync_datagrams uint8 [sync_slots, P, S, stride], sync_lengths int32 [sync_slots, P, S],
          sync_counts int32 [P, S]: the handshake's messages, to be concatenated to build_datagrams'
          along the slot axis
      events uint8 [P, S], sync_count int32 [P, S] -> events()
      liveness_received uint8 [P, S] -> P2PSession.poll_liveness' received
      send_queue_len int32 [P, S] -> network_stats()
      session_running uint8 [S] -> the run mask of P2PSession.run_ticks_paced
      status int32 [P, S]: RB_DG_NO_ROOM
    """

    def __init__(self, num_players: int, num_sessions: int, device="cuda", sync_slots: int = 4):
        import torch
        P, S, M = int(num_players), int(num_sessions), int(sync_slots)
        self.num_players, self.num_sessions, self.sync_slots = P, S, M
        self.device = torch.zeros((), device=device).device  # "cuda" -> the current device, by index
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.device)
        self.ep_state = z((P, S), torch.uint8)
        self.sync_remaining = z((P, S), torch.int32)
        self.sync_nonces = z((8, P, S), torch.int32)
        self.sync_valid = z((P, S), torch.uint8)
        self.sync_next = z((P, S), torch.uint8)
        self.stamps = z((L.RB_EP_STAMPS, P, S), torch.int64)
        self.packets_sent = z((P, S), torch.int64)
        self.last_newest = z((P, S), torch.int32)
        self.remote_magic = z((P, S), torch.int16)
        self.input_lengths = z((P, S), torch.int32)
        self.ack_due = z((P, S), torch.uint8)
        self.reply_due = z((P, S), torch.uint8)
        self.report_due = z((P, S), torch.uint8)
        self.keepalive_due = z((P, S), torch.uint8)
        self.sync_datagrams = None  # takes the stride of the first poll's datagrams
        self.sync_lengths = z((M, P, S), torch.int32)
        self.sync_counts = z((P, S), torch.int32)
        self.events_mask = z((P, S), torch.uint8)
        self.sync_count = z((P, S), torch.int32)
        self.liveness_received = z((P, S), torch.uint8)
        self.send_queue_len = z((P, S), torch.int32)
        self.session_running = z((S,), torch.uint8)
        self.status = z((P, S), torch.int32)
        self._null_frames = torch.full((P, S), L.RB_NULL_FRAME, dtype=torch.int32, device=self.device)

    def poll(self, handle_mask: int, now_ms: int, local_magic, datagrams, dg_lengths, nonces=None, start=None,
             disconnected=None, ack_owed=None, reply_owed=None, received=None, newest=None, acked=None, lengths=None,
             reports=None):
        """One poll_remote_clients and the frame's sends that follow it, for every endpoint of
        `handle_mask`: the datagrams of this poll ([M, P, S, stride] / [M, P, S], as parse_datagrams
        takes them), the caller's clock, and what parse, decode, liveness, the local-input export and
        the encoder produced (see include/ggrs_amd.h; a tensor left None means none or zero; newest
        and acked default to NULL_FRAME).  nonces: 32-bit [M, P, S], drawn with torch.randint when
        None.  Returns self."""
        import torch
        M, P, S, stride = _shape(datagrams, dg_lengths)
        assert (P, S) == (self.num_players, self.num_sessions) and datagrams.device == self.device
        dev = self.device
        if nonces is None:
            nonces = torch.randint(-2**31, 2**31, (M, P, S), dtype=torch.int32, device=dev)
        if self.sync_datagrams is None or self.sync_datagrams.shape[3] != stride:
            self.sync_datagrams = torch.zeros((self.sync_slots, P, S, stride), dtype=torch.uint8, device=dev)
        newest = self._null_frames if newest is None else newest
        acked = self._null_frames if acked is None else acked
        K = L.RB_P2P_REPORTS_PER_TAKE
        _rows(P, S, dev, local_magic=(local_magic, (P, S), 2), nonces=(nonces, (M, P, S), 4), start=(start, (P, S), 1),
              disconnected=(disconnected, (P, S), 1), ack_owed=(ack_owed, (P, S), 1), reply_owed=(reply_owed, (P, S), 1),
              received=(received, (P, S), 1), newest=(newest, (P, S), 4), acked=(acked, (P, S), 4),
              lengths=(lengths, (P, S), 4), reports=(reports, (K, S, REPORT_WORDS), 8))
        io = L.RbEndpointProtocol(
            ep_state=_ptr(self.ep_state), sync_remaining=_ptr(self.sync_remaining), sync_nonces=_ptr(self.sync_nonces),
            sync_valid=_ptr(self.sync_valid), sync_next=_ptr(self.sync_next), stamps=_ptr(self.stamps),
            packets_sent=_ptr(self.packets_sent), last_newest=_ptr(self.last_newest), remote_magic=_ptr(self.remote_magic),
            now_ms=int(now_ms), local_magic=_ptr(local_magic), start=_opt(start), datagrams=_ptr(datagrams), stride=stride,
            slots=M, sync_slots=self.sync_slots, dg_lengths=_ptr(dg_lengths), nonces=_ptr(nonces),
            disconnected=_opt(disconnected), ack_owed=_opt(ack_owed), reply_owed=_opt(reply_owed), received=_opt(received),
            newest=_ptr(newest), acked=_ptr(acked), lengths=_opt(lengths), reports=_opt(reports),
            input_lengths=_ptr(self.input_lengths), ack_due=_ptr(self.ack_due), reply_due=_ptr(self.reply_due),
            report_due=_ptr(self.report_due), keepalive_due=_ptr(self.keepalive_due),
            sync_datagrams=_ptr(self.sync_datagrams), sync_lengths=_ptr(self.sync_lengths), sync_counts=_ptr(self.sync_counts),
            events=_ptr(self.events_mask), sync_count=_ptr(self.sync_count), liveness_received=_ptr(self.liveness_received),
            send_queue_len=_ptr(self.send_queue_len), session_running=_ptr(self.session_running), status=_ptr(self.status))
        stream = torch.cuda.current_stream(dev).cuda_stream
        _call(L.load().rb_endpoint_protocol_poll_all, dev.index or 0, ctypes.c_void_p(stream), int(handle_mask), P, S,
              ctypes.byref(io))
        return self

    def reset(self, sessions) -> None:
        """Fresh endpoints for `sessions` (indices or a bool mask [S]): their columns are zeroed, as
        restart_sessions does for the batch's own planes."""
        for name in STATE_TENSORS:
            getattr(self, name)[..., sessions] = 0

    def state_dict(self, sessions=None) -> dict:
        """The state tensors, or copies of the columns of `sessions`: with the same indices
        move_sessions takes, a moved session's endpoints travel by plain indexing."""
        return {name: getattr(self, name) if sessions is None else getattr(self, name)[..., sessions].clone()
                for name in STATE_TENSORS}

    def load_state_dict(self, state: dict, sessions=None) -> None:
        """Write `state` (a state_dict) into every column, or into the columns of `sessions`."""
        for name in STATE_TENSORS:
            if sessions is None:
                getattr(self, name).copy_(state[name])
            else:
                getattr(self, name)[..., sessions] = state[name].to(self.device)

    def events(self) -> list:
        """The last poll's events per session: ("Synchronizing", handle, total, count) and
        ("Synchronized", handle), handles ascending.  Synchronises."""
        ev, count = self.events_mask.cpu().numpy(), self.sync_count.cpu().numpy()
        out = [[] for _ in range(self.num_sessions)]
        for h, s in zip(*ev.nonzero()):
            if ev[h, s] & L.RB_EP_EVENT_SYNCHRONIZING:
                out[s].append(("Synchronizing", int(h), NUM_SYNC_PACKETS, int(count[h, s])))
            if ev[h, s] & L.RB_EP_EVENT_SYNCHRONIZED:
                out[s].append(("Synchronized", int(h)))
        return out

    def network_stats(self, now_ms: int, message_bytes: int) -> dict:
        """The send half of UdpProtocol::network_stats (protocol.rs:279-301) per endpoint, as numpy
        [P, S]: send_queue_len of the last poll and kbps_sent = ((packets_sent * (message_bytes +
        28)) / seconds) / 1024 in integers, seconds = (now_ms - stats_start) / 1000.  message_bytes is
        the reference build's size_of::<Message>(), which only that build knows.  kbps_sent is -1
        (NotSynchronized) where seconds is 0 or the endpoint is neither Synchronizing nor Running.
        Synchronises."""
        import numpy as np
        state = self.ep_state.cpu().numpy()
        sent = self.packets_sent.cpu().numpy()
        seconds = (int(now_ms) - self.stamps[4].cpu().numpy()) // 1000
        ok = ((state == L.RB_EP_SYNCHRONIZING) | (state == L.RB_EP_RUNNING)) & (seconds > 0)
        kbps = np.where(ok, sent * (int(message_bytes) + UDP_HEADER_SIZE) // np.where(ok, seconds, 1) // 1024, -1)
        return {"send_queue_len": self.send_queue_len.cpu().numpy(), "kbps_sent": kbps.astype(np.int64)}

    def gate(self, out_lengths, out_counts) -> None:
        """After build_datagrams: empty the rows of endpoints in Shutdown, which send nothing
        (protocol.rs:429-432); build has no per-endpoint gate for a session's checksum reports."""
        live = self.ep_state < L.RB_EP_SHUTDOWN
        out_lengths.mul_(live.to(out_lengths.dtype))
        out_counts.mul_(live.to(out_counts.dtype))
