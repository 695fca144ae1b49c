"""The caller's side of a per-session delivery ring (include/ggrs_amd.h
rb_p2p_set_delivery_ring).

A batch in ring mode reads its remote inputs from a tensor [R, P, S] in which
frame f of session s sits in slot f & (R - 1): every session counts frames from
its own match's start, so sessions that restarted or were imported at different
times share one tensor of R frames.  ``DeliveryRing`` holds that tensor and the
per-endpoint watermark (the newest frame delivered, what UdpProtocol's
Event::Input stream has handed over, p2p_session.rs:838-852), and scatters
newly arrived frames into their slots with torch on the device: no host loop
over sessions, and ``scatter`` does not synchronise (``restart`` and
``move_columns``, called when matches begin or move, may: a boolean mask or a
host index list goes through the host).

Over a real link the frames arrive as packets: ``receive_packets`` decodes every
endpoint's packet into its slots and advances the watermarks in one launch, and
``send_packets`` encodes out of a ring that ``export_local_inputs`` or
``export_confirmed_inputs`` filled (rb_decode_input_packets_all,
rb_encode_input_packets_all).
"""
from __future__ import annotations

from . import _lib as L


class DeliveryRing:
    """inputs [R, P, S] (the remote_inputs / host_inputs / inputs_by_frame argument of a batch
    in ring mode) and upto [P, S] int32 (a tick's remote_upto row; NULL_FRAME: nothing yet)."""

    def __init__(self, ring_frames: int, num_players: int, num_sessions: int, dtype=None, device="cuda"):
        import torch
        R = int(ring_frames)
        if R < L.RB_INPUT_QUEUE_LENGTH or R & (R - 1):
            raise ValueError("ring_frames is a power of two of at least 128")
        self.ring_frames, self.num_players, self.num_sessions = R, int(num_players), int(num_sessions)
        self.inputs = torch.zeros((R, self.num_players, self.num_sessions), dtype=dtype or torch.uint8, device=device)
        # 2-byte inputs serve the packet codec (receive_packets / send_packets); the batches
        # themselves take inputs of 1 or 4 bytes
        if self.inputs.element_size() not in (1, 2, 4):
            raise ValueError("inputs of 1, 2 or 4 bytes")
        self.upto = torch.full((self.num_players, self.num_sessions), L.RB_NULL_FRAME, dtype=torch.int32, device=device)
        self._cols = torch.arange(self.num_sessions, device=device)

    def _raw(self, x):
        """4- and 2-byte inputs as int32 / int16 (torch indexes few unsigned types); the bits are what counts."""
        import torch
        return x.view({4: torch.int32, 2: torch.int16}[x.element_size()]) if x.element_size() != 1 else x

    def scatter(self, handle: int, first, count, values) -> None:
        """The frames that arrived for `handle`: session s got frames first[s] .. first[s] +
        count[s] - 1, values[k, s] being frame first[s] + k (rows k >= count[s] are ignored).
        first, count int32 [S] and values [K, S] are tensors on the ring's device, K <= R.  The
        watermark of every session with count > 0 moves up to its last frame (never down)."""
        import torch
        K = int(values.shape[0])
        assert K <= self.ring_frames, "one scatter writes no slot twice"
        assert tuple(values.shape) == (K, self.num_sessions) and values.element_size() == self.inputs.element_size()
        assert tuple(first.shape) == tuple(count.shape) == (self.num_sessions,)
        k = torch.arange(K, device=self.inputs.device)[:, None]
        first, count = first.to(torch.int64), count.to(torch.int64)
        slot = (first[None, :] + k) & (self.ring_frames - 1)
        cols = self._cols[None, :].expand(K, -1)
        plane = self._raw(self.inputs)[:, int(handle), :]
        # rows past a session's count rewrite what their slot holds (distinct slots per column)
        plane[slot, cols] = torch.where(k < count[None, :], self._raw(values), plane[slot, cols])
        last = torch.where(count > 0, first + count - 1, torch.full_like(first, L.RB_NULL_FRAME)).to(torch.int32)
        self.upto[int(handle)] = torch.maximum(self.upto[int(handle)], last)

    def _groups(self, handle_mask, groups):
        from .endpoint_groups import as_groups
        g = as_groups(groups, self.num_players)
        if handle_mask is not None and int(handle_mask) != g.lead_mask:
            raise ValueError("with groups, handle_mask is omitted or the groups' lead mask")
        return g

    def receive_packets(self, handle_mask, packets, lengths, start_frames, max_prediction: int, status=None, groups=None):
        """UdpProtocol::on_input for every endpoint of the handles in handle_mask, in one launch
        (wire.decode_packets in ring mode): packets uint8 [P, S, stride], lengths and start_frames
        int32 [P, S].  New frames go to their slots and ``upto`` advances; a packet with more than R
        new frames is taken up to R of them (the sender, acked with ``upto``, sends the rest again).
        The batch must have consumed every frame up to ``upto`` before the call.  Returns the status
        tensor [P, S] (0 new inputs, 1 nothing new, -1 malformed, -2 a gap; rows outside the mask
        are left alone).  With `groups` (an EndpointGroups, or a sequence of handle sequences or
        masks) every endpoint carries its group's handles in one stream (rb_decode_input_packets_grouped,
        DESIGN.md section 21): the rows read are the leads', every member's inputs and ``upto`` row
        are written, and handle_mask is None or the groups' lead mask.  Does not synchronise."""
        from .wire import decode_packets, decode_packets_grouped
        if groups is not None:
            return decode_packets_grouped(self.inputs, self.upto, self._groups(handle_mask, groups), packets, lengths,
                                          start_frames, max_prediction, status=status, ring_frames=self.ring_frames)
        return decode_packets(self.inputs, self.upto, handle_mask, packets, lengths, start_frames, max_prediction,
                              status=status, ring_frames=self.ring_frames)

    def send_packets(self, handle_mask, newest, acked, first_frame: int, packets, lengths, start_frames, groups=None) -> None:
        """UdpProtocol::send_pending_output for every endpoint of the handles in handle_mask, in one
        launch (wire.encode_packets in ring mode), with this ring holding the sender's inputs (the
        tensor of export_local_inputs or export_confirmed_inputs): frames acked + 1 .. newest
        (first_frame .. newest before any ack) against the input of frame acked.  newest and acked
        int32 [P, S] (`sent` of export_local_inputs; the receiver's ``upto`` as it came back).
        lengths: bytes, 0 nothing pending, -1 longer than the stride, -2 more than R frames from the
        ack to newest (the reference input is gone; the reference disconnects such an endpoint).
        With `groups` the frames of every member of a group go into one packet in the lead's row
        (rb_encode_input_packets_grouped); handle_mask is None or the groups' lead mask.
        Does not synchronise."""
        from .wire import encode_packets, encode_packets_grouped
        if groups is not None:
            return encode_packets_grouped(self.inputs, self._groups(handle_mask, groups), newest, acked, first_frame,
                                          packets, lengths, start_frames, ring_frames=self.ring_frames)
        encode_packets(self.inputs, handle_mask, newest, acked, first_frame, packets, lengths, start_frames,
                       ring_frames=self.ring_frames)

    def restart(self, sessions) -> None:
        """The sessions (a bool / index tensor or array) begin a new match: their watermarks are
        NULL_FRAME again.  Their columns keep the old match's inputs, which are never read."""
        import torch
        self.upto[:, torch.as_tensor(sessions, device=self.upto.device)] = L.RB_NULL_FRAME

    def move_columns(self, src: "DeliveryRing", src_sessions, dst_sessions) -> None:
        """The ring columns and watermarks of sessions that moved from `src`'s batch into this
        one's (move_sessions): a moved session keeps its own frame numbering."""
        import torch
        assert self.ring_frames == src.ring_frames
        a = torch.as_tensor(src_sessions, device=self.upto.device, dtype=torch.int64)
        b = torch.as_tensor(dst_sessions, device=self.upto.device, dtype=torch.int64)
        self._raw(self.inputs)[:, :, b] = self._raw(src.inputs)[:, :, a]
        self.upto[:, b] = src.upto[:, a]
