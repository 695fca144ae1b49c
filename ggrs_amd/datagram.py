"""GGRS's wire messages over tensors (include/ggrs_amd.h rb_parse_datagrams_all,
rb_build_datagrams_all): the datagrams an unmodified GGRS
peer puts on its socket, Message { header: { magic }, body } under bincode,
parsed and built for every endpoint of a batch in one launch each.

The endpoint of handle h, session s owns row (h, s) of every [P, S] tensor, as
in ggrs_amd.wire; rows of handles outside handle_mask are untouched.  Datagrams
are uint8 [M, P, S, stride] (M slots per endpoint, 1..8; stride a multiple of
16 of at least 64) with int32 [M, P, S] lengths.  Both calls run on the current
torch stream and neither synchronises; a refused request raises InvalidRequest
before anything runs.
"""
from __future__ import annotations

import ctypes

from . import _lib as L
from .wire import _call, _ptr

REPORT_WORDS = 3  # rb_checksum_report as int64 words: checksum lo, hi, frame | mismatch_frame << 32


def _opt(t):
    return None if t is None else _ptr(t)


class ParsedDatagrams:
    """Every tensor rb_parse_datagrams_all writes, for P players and S sessions, laid out for the
    calls that take them:
      received, disconnect_requested  uint8 [P, S]      -> P2PSession.poll_liveness
      acked                           int32 [P, S]      -> encode_packets' acked (in/out, starts NULL_FRAME)
      peer_last_frames / peer_disconnected  int32 / uint8 [P, P, S]; row h -> receive_peer_connect_status(h, ...)
      packets, lengths, start_frames  uint8 [P, S, packet_stride], int32 [P, S] -> decode_packets
      frame_advantage, rtt_ms         int32 [P, S] (in/out) -> receive_quality(h, rtt_ms[h], frame_advantage[h])
      reply_owed, reply_ping          uint8 [P, S], int64 [2, P, S] (the u128's low and high words) -> build_datagrams
      reports, report_counts          int64 [P, K, S, 3], int32 [P, S] (in/out); reports[h] ->
                                      receive_checksum_reports(h, ...), then report_counts[h] = 0
      status                          int32 [P, S] RB_DG_* bits
    """

    def __init__(self, num_players: int, num_sessions: int, packet_stride: int = 64, device="cuda"):
        import torch
        P, S, K = int(num_players), int(num_sessions), L.RB_P2P_REPORTS_PER_TAKE
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
        self.num_players, self.num_sessions = P, S
        self.received = z((P, S), torch.uint8)
        self.disconnect_requested = z((P, S), torch.uint8)
        self.acked = torch.full((P, S), L.RB_NULL_FRAME, dtype=torch.int32, device=device)
        self.peer_last_frames = torch.full((P, P, S), L.RB_NULL_FRAME, dtype=torch.int32, device=device)
        self.peer_disconnected = z((P, P, S), torch.uint8)
        self.packets = z((P, S, int(packet_stride)), torch.uint8)
        self.lengths = z((P, S), torch.int32)
        self.start_frames = z((P, S), torch.int32)
        self.frame_advantage = z((P, S), torch.int32)
        self.reply_owed = z((P, S), torch.uint8)
        self.reply_ping = z((2, P, S), torch.int64)
        self.rtt_ms = z((P, S), torch.int32)
        self.reports = z((P, K, S, REPORT_WORDS), torch.int64)
        self.reports[..., 2] = -1
        self.report_counts = z((P, S), torch.int32)
        self.status = z((P, S), torch.int32)

    def tensors(self):
        return {k: v for k, v in vars(self).items() if hasattr(v, "data_ptr")}


def _shape(datagrams, lengths):
    import torch
    assert datagrams.dtype == torch.uint8 and datagrams.dim() == 4 and datagrams.is_contiguous() and datagrams.is_cuda
    M, P, S, stride = datagrams.shape
    assert lengths.dtype == torch.int32 and tuple(lengths.shape) == (M, P, S) and lengths.is_contiguous()
    return int(M), int(P), int(S), int(stride)


def _rows(P, S, device, **tensors):
    for name, (t, shape, size) in tensors.items():
        if t is None:
            continue
        assert tuple(t.shape) == shape and t.element_size() == size and t.is_contiguous() and t.device == device, name


def parse_datagrams(out: ParsedDatagrams, handle_mask: int, datagrams, dg_lengths, remote_magic, now_ms: int):
    """UdpProtocol::handle_message for every endpoint of `handle_mask`: the datagrams of this poll,
    in slot order, into `out` (see ParsedDatagrams).  remote_magic: a 16-bit tensor [P, S], 0 accepts
    any magic; now_ms: the caller's epoch clock.  Returns `out`."""
    import torch
    M, P, S, stride = _shape(datagrams, dg_lengths)
    assert (P, S) == (out.num_players, out.num_sessions)
    dev = datagrams.device
    _rows(P, S, dev, remote_magic=(remote_magic, (P, S), 2))
    for t in out.tensors().values():
        assert t.device == dev and t.is_contiguous()
    io = L.RbDatagramParse(
        datagrams=_ptr(datagrams), stride=stride, slots=M, dg_lengths=_ptr(dg_lengths), remote_magic=_ptr(remote_magic),
        now_ms=int(now_ms), received=_ptr(out.received), disconnect_requested=_ptr(out.disconnect_requested),
        acked=_ptr(out.acked), peer_last_frames=_ptr(out.peer_last_frames), peer_disconnected=_ptr(out.peer_disconnected),
        packets=_ptr(out.packets), packet_stride=int(out.packets.shape[2]), lengths=_ptr(out.lengths),
        start_frames=_ptr(out.start_frames), frame_advantage=_ptr(out.frame_advantage), reply_owed=_ptr(out.reply_owed),
        reply_ping=_ptr(out.reply_ping), rtt_ms=_ptr(out.rtt_ms), reports=_ptr(out.reports),
        report_counts=_ptr(out.report_counts), status=_ptr(out.status))
    stream = torch.cuda.current_stream(dev).cuda_stream
    _call(L.load().rb_parse_datagrams_all, dev.index or 0, ctypes.c_void_p(stream), int(handle_mask), P, S, ctypes.byref(io))
    return out


def build_datagrams(handle_mask: int, out_datagrams, out_lengths, out_counts, status, local_magic, now_ms: int, ack_frame,
                    status_last_frames, status_disconnected, packets=None, lengths=None, start_frames=None,
                    disconnect_requested=None, ack_owed=None, reply_owed=None, reply_ping=None, report_due=None,
                    frame_advantage=None, reports=None, keepalive_due=None) -> None:
    """The datagrams every endpoint of `handle_mask` owes this poll, densely packed in priority
    order into out_datagrams [M, P, S, stride] / out_lengths [M, P, S] / out_counts [P, S]: Input
    (packets / lengths / start_frames as encode_packets wrote them, ack_frame, disconnect_requested,
    the sender's connect status [P, S]), InputAck (ack_owed), QualityReply (reply_owed, reply_ping
    [2, P, S]), QualityReport (report_due, frame_advantage, ping = now_ms), ChecksumReports
    (reports [K, S, 3], take_checksum_reports' tensor) and KeepAlive (keepalive_due, only when
    nothing else was written).  A tensor left None means none due.  status [P, S] gets RB_DG_* bits."""
    import torch
    M, P, S, stride = _shape(out_datagrams, out_lengths)
    dev = out_datagrams.device
    K = L.RB_P2P_REPORTS_PER_TAKE
    _rows(P, S, dev, out_counts=(out_counts, (P, S), 4), status=(status, (P, S), 4), local_magic=(local_magic, (P, S), 2),
          ack_frame=(ack_frame, (P, S), 4), status_last_frames=(status_last_frames, (P, S), 4),
          status_disconnected=(status_disconnected, (P, S), 1), lengths=(lengths, (P, S), 4),
          start_frames=(start_frames, (P, S), 4), disconnect_requested=(disconnect_requested, (P, S), 1),
          ack_owed=(ack_owed, (P, S), 1), reply_owed=(reply_owed, (P, S), 1), reply_ping=(reply_ping, (2, P, S), 8),
          report_due=(report_due, (P, S), 1), frame_advantage=(frame_advantage, (P, S), 4),
          reports=(reports, (K, S, REPORT_WORDS), 8), keepalive_due=(keepalive_due, (P, S), 1))
    packet_stride = 0
    if packets is not None:
        assert packets.dtype == torch.uint8 and packets.is_contiguous() and tuple(packets.shape[:2]) == (P, S)
        assert lengths is not None and start_frames is not None
        packet_stride = int(packets.shape[2])
    io = L.RbDatagramBuild(
        local_magic=_ptr(local_magic), now_ms=int(now_ms), packets=_opt(packets), packet_stride=packet_stride,
        lengths=_opt(lengths), start_frames=_opt(start_frames), ack_frame=_ptr(ack_frame),
        disconnect_requested=_opt(disconnect_requested), status_last_frames=_ptr(status_last_frames),
        status_disconnected=_ptr(status_disconnected), ack_owed=_opt(ack_owed), reply_owed=_opt(reply_owed),
        reply_ping=_opt(reply_ping), report_due=_opt(report_due), frame_advantage=_opt(frame_advantage),
        reports=_opt(reports), keepalive_due=_opt(keepalive_due), out_datagrams=_ptr(out_datagrams), stride=stride, slots=M,
        out_lengths=_ptr(out_lengths), out_counts=_ptr(out_counts), status=_ptr(status))
    stream = torch.cuda.current_stream(dev).cuda_stream
    _call(L.load().rb_build_datagrams_all, dev.index or 0, ctypes.c_void_p(stream), int(handle_mask), P, S, ctypes.byref(io))
