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
        if self.inputs.element_size() not in (1, 4):
            raise ValueError("inputs of 1 or 4 bytes")
        self.upto = torch.full((self.num_players, self.num_sessions), L.RB_NULL_FRAME, dtype=torch.int32, device=device)
        self._cols = torch.arange(self.num_sessions, device=device)

    def _raw(self, x):
        """4-byte inputs as int32 (torch indexes few unsigned types); the bits are what counts."""
        import torch
        return x.view(torch.int32) if x.element_size() == 4 else x

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
