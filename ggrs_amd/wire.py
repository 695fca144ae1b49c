"""The packet codec over tensors (include/ggrs_amd.h rb_decode_input_packets_all,
rb_encode_input_packets_all): UdpProtocol::on_input and
send_pending_output for every endpoint of a batch in one launch, into and out
of a linear [frames, P, S] tensor or a delivery ring [R, P, S].

The endpoint of handle h, session s owns row (h, s) of every tensor: packets
uint8 [P, S, stride] (stride a multiple of 16, at least 32), lengths and
start_frames int32 [P, S] (one tick of run_ticks_packets' layout), and upto /
status / acked / newest int32 [P, S].  Rows of handles outside handle_mask are
untouched.  Both calls run on the current torch stream and neither
synchronises; a refused request raises InvalidRequest before anything runs.
"""
from __future__ import annotations

import ctypes

from . import _lib as L


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _check(inputs, handle_mask, packets, per_endpoint):
    import torch
    assert inputs.dim() == 3 and inputs.is_contiguous() and inputs.is_cuda
    _, P, S = inputs.shape
    assert packets.dtype == torch.uint8 and packets.is_contiguous() and tuple(packets.shape[:2]) == (P, S)
    for t in per_endpoint:
        assert t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (P, S) and t.device == inputs.device
    return P, S, int(packets.shape[2])


def _call(fn, *args):
    from .session import DeviceError, InvalidRequest
    st = fn(*args)
    if st == L.RB_INVALID_REQUEST:
        raise InvalidRequest(f"{fn.__name__}: see include/ggrs_amd.h for the shapes it takes")
    if st != L.RB_OK:
        raise DeviceError(f"{fn.__name__}: rb_status {st}")


def decode_packets(inputs, upto, handle_mask: int, packets, lengths, start_frames, max_prediction: int,
                   status=None, ring_frames: int = 0):
    """Decode every endpoint's packet into `inputs` ([frames, P, S], or the ring [R, P, S] with
    ring_frames = R) and advance `upto`.  Returns the status tensor (0 new inputs, 1 nothing new,
    -1 malformed, -2 frames missing before the start frame), `status` itself when given."""
    import torch
    if status is None:
        status = torch.zeros_like(upto)
    P, S, stride = _check(inputs, handle_mask, packets, (lengths, start_frames, upto, status))
    stream = torch.cuda.current_stream(inputs.device).cuda_stream
    _call(L.load().rb_decode_input_packets_all, inputs.device.index or 0, ctypes.c_void_p(stream), int(handle_mask), P, S,
          inputs.element_size(), int(max_prediction), _ptr(packets), stride, _ptr(lengths), _ptr(start_frames),
          _ptr(inputs), int(inputs.shape[0]), int(ring_frames), _ptr(upto), _ptr(status))
    return status


def encode_packets(inputs, handle_mask: int, newest, acked, first_frame: int, packets, lengths, start_frames,
                   ring_frames: int = 0) -> None:
    """Encode, per endpoint, the inputs of frames acked + 1 .. newest (first_frame .. newest before
    any ack) from `inputs` against the input of frame acked.  lengths: the packet's bytes, 0
    nothing pending, -1 longer than the stride, -2 (ring) the reference input was overwritten."""
    import torch
    P, S, stride = _check(inputs, handle_mask, packets, (lengths, start_frames, acked, newest))
    stream = torch.cuda.current_stream(inputs.device).cuda_stream
    _call(L.load().rb_encode_input_packets_all, inputs.device.index or 0, ctypes.c_void_p(stream), int(handle_mask), P, S,
          inputs.element_size(), _ptr(inputs), int(inputs.shape[0]), int(ring_frames), int(first_frame), _ptr(acked),
          _ptr(newest), _ptr(packets), stride, _ptr(lengths), _ptr(start_frames))


def decode_packets_grouped(inputs, upto, groups, packets, lengths, start_frames, max_prediction: int,
                           status=None, ring_frames: int = 0):
    """decode_packets for endpoints that carry a group of handles in one stream (`groups`: an
    EndpointGroups or what it takes; rb_decode_input_packets_grouped).  The
    packet, length, start frame and status are the lead's rows; every member's column of `inputs`
    and row of `upto` is written."""
    import torch
    from .endpoint_groups import as_groups
    if status is None:
        status = torch.zeros_like(upto)
    P, S, stride = _check(inputs, 0, packets, (lengths, start_frames, upto, status))
    stream = torch.cuda.current_stream(inputs.device).cuda_stream
    _call(L.load().rb_decode_input_packets_grouped, inputs.device.index or 0, ctypes.c_void_p(stream),
          as_groups(groups, P).packed, P, S, inputs.element_size(), int(max_prediction), _ptr(packets), stride,
          _ptr(lengths), _ptr(start_frames), _ptr(inputs), int(inputs.shape[0]), int(ring_frames), _ptr(upto), _ptr(status))
    return status


def encode_packets_grouped(inputs, groups, newest, acked, first_frame: int, packets, lengths, start_frames,
                           ring_frames: int = 0) -> None:
    """encode_packets for endpoints that carry a group of handles in one stream: acked and newest
    are the lead's rows, the frames come from every member's column, the packet goes to the lead's
    row (rb_encode_input_packets_grouped)."""
    import torch
    from .endpoint_groups import as_groups
    P, S, stride = _check(inputs, 0, packets, (lengths, start_frames, acked, newest))
    stream = torch.cuda.current_stream(inputs.device).cuda_stream
    _call(L.load().rb_encode_input_packets_grouped, inputs.device.index or 0, ctypes.c_void_p(stream),
          as_groups(groups, P).packed, P, S, inputs.element_size(), _ptr(inputs), int(inputs.shape[0]), int(ring_frames),
          int(first_frame), _ptr(acked), _ptr(newest), _ptr(packets), stride, _ptr(lengths), _ptr(start_frames))
