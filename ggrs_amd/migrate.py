"""Moving running sessions between batches (include/ggrs_amd.h rb_p2p_export_sessions,
rb_p2p_import_sessions and the spectators' twins).

GGRS has no such call: a P2PSession is an ordinary movable Rust value.  Here a session is a
column of its batch, exported as a session record: a position-independent byte image that can be
imported into any column of a batch of the same configuration, on this device or another, now or
after a process restart."""
import ctypes

import numpy as np


class _Movable:
    """export_sessions / import_sessions of a batch class whose C calls begin with _MOVE (mixed
    into a _StreamOrdered class)."""

    _MOVE = ""

    def _move_fn(self, name):
        return getattr(self._lib, f"{self._MOVE}_{name}")

    def _session_list(self, sessions):
        idx = np.ascontiguousarray(np.asarray(sessions).reshape(-1), dtype=np.int32)
        return idx, idx.ctypes.data_as(ctypes.c_void_p)

    @property
    def record_bytes(self) -> int:
        """Bytes of one session record: a function of the batch's configuration alone."""
        return int(self._move_fn("session_record_bytes")(self._h))

    def export_sessions(self, sessions, out=None):
        """The sessions `sessions` (distinct indices) as records: a torch.uint8 [n, record_bytes]
        tensor on the batch's device, record k of sessions[k].  Stream ordered, between ticks; the
        batch is only read.  out: a contiguous tensor of that shape to write into (its padding
        bytes stay as they are) instead of a new, zeroed one."""
        import torch
        idx, ptr = self._session_list(sessions)
        dev = torch.device("cuda", self._device)
        shape = (len(idx), self.record_bytes)
        if out is None:
            records = torch.zeros(shape, dtype=torch.uint8, device=dev)
        else:
            if out.dtype != torch.uint8 or out.device != dev or tuple(out.shape) != shape or not out.is_contiguous():
                raise ValueError(f"out must be a contiguous torch.uint8 tensor {shape} on the batch's device")
            records = out
        cur = self._pre()
        st = self._move_fn("export_sessions")(self._h, ptr, len(idx), ctypes.c_void_p(records.data_ptr()))
        self._post(cur, (records,), outputs=True)
        self._check(st)
        return records

    def import_sessions(self, sessions, records) -> None:
        """Records [n, record_bytes] (torch.uint8, on the batch's device) into the sessions
        `sessions`: record k becomes session sessions[k], which continues the match the record
        was exported from; hand it that match's tensor columns from now on.  A record of another
        configuration leaves its session untouched and counts in import_refused()."""
        import torch
        idx, ptr = self._session_list(sessions)
        if not isinstance(records, torch.Tensor) or not records.is_cuda or records.dtype != torch.uint8:
            raise TypeError("records must be a torch.uint8 CUDA tensor")
        if records.device.index != self._device:
            raise ValueError("records must be on the batch's device (move_sessions copies them across)")
        if tuple(records.shape) != (len(idx), self.record_bytes):
            raise ValueError(f"records must be [{len(idx)}, {self.record_bytes}], not {tuple(records.shape)}")
        records = records.contiguous()
        cur = self._pre()
        st = self._move_fn("import_sessions")(self._h, ptr, len(idx), ctypes.c_void_p(records.data_ptr()))
        self._post(cur, (records,))
        self._check(st)

    def import_refused(self) -> int:
        """Records import_sessions refused since create (synchronises)."""
        n = ctypes.c_uint32()
        self._check(self._move_fn("import_refused")(self._h, ctypes.byref(n)))
        return int(n.value)


def move_sessions(src, src_sessions, dst, dst_sessions):
    """Sessions src_sessions of batch `src` become sessions dst_sessions of batch `dst` (the same
    kind of batch, the same configuration; the k-th to the k-th): export, a copy of the records to
    dst's device if it is another, import.  Returns the records as imported.  `src` is left as it
    was: restart or overwrite its columns, and move the caller's tensor columns alike."""
    if len(np.asarray(src_sessions).reshape(-1)) != len(np.asarray(dst_sessions).reshape(-1)):
        raise ValueError("as many destination sessions as source sessions")
    records = src.export_sessions(src_sessions)
    if src._device != dst._device:
        import torch
        records = records.to(torch.device("cuda", dst._device))
    dst.import_sessions(dst_sessions, records)
    return records
