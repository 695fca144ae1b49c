"""The packet codec for delivery rings (include/ggrs_amd.h rb_decode_input_packets_all,
rb_encode_input_packets_all; ggrs_amd.wire; DeliveryRing.receive_packets / send_packets; DESIGN.md
section 17): UdpProtocol::on_input and send_pending_output for every endpoint of a batch in one
launch, into and out of a ring [R, P, S] in which frame f sits in slot f & (R - 1).

Every expectation comes from a small model of on_input / send_pending_output over a ring
(``model_decode`` / ``model_encode``), built on test_wire.on_input_reference, oracle.wire_encode and
oracle.wire_decode; all comparisons are equalities.  The seeded schedules (``decode_case``,
``encode_case``) give every endpoint one of a fixed list of situations; a CPU witness counts, on the
model alone, that every situation the kernels can get wrong is in them.

S = 200 for the codec tests (three full waves and a ragged one), S = 70 for the closed loops,
R = 128, W = 8.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine library is loaded: the process then holds one HIP runtime, torch's)

import ggrs_amd as G
from ggrs_amd import _lib as L
from ggrs_amd.p2p import synth_network
from ggrs_amd.wire import decode_packets, encode_packets
from ggrs_amd.synth import SEED
from oracle import oracle as O
from test_wire import on_input_reference, rand_inputs
from test_wire_edges import TABLE, block_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, W, S, SL = 128, 8, 200, 70
M = R - 1
STRIDE = 160         # the decode tests' packet rows
ROOMY, TIGHT = 544, 32  # the encode tests' rows: every packet fits / the shortest legal row
CASES = [(2, 0b10), (4, 0b1110), (4, 0b1010)]  # (P, handle mask)
SENT = -77           # what rows and entries nobody may write are prefilled with


def handles_of(mask, P):
    return [h for h in range(P) if (mask >> h) & 1]


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def model_decode(raw, upto, status, mask, pk, ln, st):
    """on_input for every endpoint of the mask over a ring.  raw uint8 [R, P, S, ib], upto and
    status int32 [P, S], pk uint8 [P, S, stride], ln / st int32 [P, S]: updated in place.  Returns
    {(h, s): (first new frame, last new frame, new frames the packet carried)} of the endpoints
    that took inputs."""
    F, P, n, ib = raw.shape
    stride = pk.shape[2]
    took = {}
    for h in handles_of(mask, P):
        for s in range(n):
            last, start, k = int(upto[h, s]), int(st[h, s]), int(ln[h, s])
            if k > stride:  # the row does not hold the datagram
                status[h, s] = -1
                continue
            refin = raw[(start - 1) & (F - 1), h, s].tobytes()
            out, nl, code = on_input_reference(last, start, pk[h, s, :max(k, 0)].tobytes(), refin, W, ib)
            if out:  # at most the first R frames above `last`: no slot twice, and upto stops there
                lo = min(out)
                keep = {f: b for f, b in out.items() if f < lo + F}
                for f, b in keep.items():
                    raw[f & (F - 1), h, s] = np.frombuffer(b, np.uint8)
                took[h, s] = (lo, max(keep), len(out))
                nl = max(keep)
            upto[h, s] = nl
            status[h, s] = code
    return took


def model_encode(raw, mask, acked, newest, first_frame, stride, ring=True):
    """send_pending_output for every endpoint of the mask: ({(h, s): packet bytes}, lengths,
    start_frames); rows outside the mask keep SENT."""
    F, P, n, ib = raw.shape
    ln = np.full((P, n), SENT, np.int32)
    st = np.full((P, n), SENT, np.int32)
    packets = {}
    for h in handles_of(mask, P):
        for s in range(n):
            a, nw = int(acked[h, s]), int(newest[h, s])
            start = first_frame if a == -1 else a + 1
            st[h, s] = start
            if nw < start or start < 0 or (not ring and nw >= F):
                ln[h, s] = 0
                continue
            if ring and nw - (start if a == -1 else a) + 1 > F:
                ln[h, s] = -2
                continue
            slot = (lambda f: f & (F - 1)) if ring else (lambda f: f)
            ref = bytes(ib) if a == -1 else raw[slot(a), h, s].tobytes()
            want = O.wire_encode(ref, raw[[slot(f) for f in range(start, nw + 1)], h, s])
            ln[h, s] = len(want) if len(want) <= stride else -1
            if len(want) <= stride:
                packets[h, s] = want
    return packets, ln, st


# ---------------------------------------------------------------------------
# the schedules
# ---------------------------------------------------------------------------
DECODE_KINDS = ["new", "wrap", "ref_top", "first", "first_neg", "stale", "edge_stale", "gap", "malformed", "overlong",
                "cap", "cap_first", "neg_ref", "run1", "run1_ff", "lit1", "long", "long_multi", "none", "new"]


def stream_bytes(rng, count, ib):
    """count inputs' worth of XOR-stream bytes in 1 .. 254: no byte a run can take."""
    return rng.integers(1, 255, (count, ib), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def decode_case(ib, P, mask, seed=0):
    """A receiver's ring, watermarks and one packet per endpoint: (raw [R, P, S, ib], upto [P, S],
    pk [P, S, STRIDE], ln, st [P, S], kinds {(h, s): name}).  The ring starts out full of an older
    match's bytes."""
    rng = np.random.default_rng(1000 * ib + 10 * P + mask + seed)
    raw = rng.integers(0, 256, (R, P, S, ib), dtype=np.uint8)
    upto = np.full((P, S), SENT, np.int32)
    pk = rng.integers(0, 256, (P, S, STRIDE), dtype=np.uint8)  # bytes past a packet's length are noise
    ln = np.full((P, S), SENT, np.int32)
    st = np.full((P, S), SENT, np.int32)
    kinds = {}
    for h in handles_of(mask, P):
        for s in range(S):
            kind = DECODE_KINDS[(s + 7 * h) % len(DECODE_KINDS)]
            kinds[h, s] = kind
            last = int(rng.integers(200, 1 << 30) - 8)
            redo = int(rng.integers(0, 3))
            vals = None       # the packet's inputs, XORed with the reference below
            xor = None        # or the XOR stream itself
            if kind == "new":
                vals = rand_inputs(rng, int(rng.integers(1, 6)) + redo, ib)
            elif kind == "wrap":
                last = int(rng.integers(2, 1 << 22)) * R + R - 3
                vals = rand_inputs(rng, 6 + redo, ib)
            elif kind == "ref_top":
                last, redo = int(rng.integers(2, 1 << 22)) * R - 1, 0
                vals = rand_inputs(rng, int(rng.integers(1, 5)), ib)
            elif kind in ("first", "first_neg", "cap_first"):
                last, redo = -1, 0
            elif kind == "neg_ref":
                last, redo = int(rng.integers(0, 5)), 0
            start = last + 1 - redo
            if kind == "first":
                start, vals = int(rng.integers(0, 4)), rand_inputs(rng, int(rng.integers(1, 6)), ib)
            elif kind == "first_neg":
                start, vals = -3, rand_inputs(rng, 6, ib)
            elif kind == "cap_first":
                start, xor = 2, np.zeros((R + 10, ib), np.uint8)
            elif kind == "neg_ref":
                start, vals = -3, rand_inputs(rng, 12, ib)
            elif kind == "stale":       # the reference is older than recv_inputs keeps; frames past `last` follow
                start, vals = last - 2 * W - int(rng.integers(1, 6)), rand_inputs(rng, 2 * W + 12, ib)
            elif kind == "edge_stale":  # exactly as old as recv_inputs still keeps
                start, vals = last - 2 * W + 1, rand_inputs(rng, 2 * W + 3, ib)
            elif kind == "gap":
                start, vals = last + 2, rand_inputs(rng, 3, ib)
            elif kind == "cap":         # more than R new frames: a run, then two literal inputs
                xor = np.concatenate([np.zeros((R + 40 + redo, ib), np.uint8), stream_bytes(rng, 2, ib)])
            elif kind in ("run1", "run1_ff"):
                count = int(rng.integers(-(-4 // ib), 31 // ib + 1))
                xor = np.full((count, ib), 0xFF if kind == "run1_ff" else 0, np.uint8)
            elif kind == "lit1":
                xor = stream_bytes(rng, int(rng.integers(1, 31 // ib + 1)), ib)
            elif kind == "long":
                xor = stream_bytes(rng, 40 // ib, ib)
            elif kind == "long_multi":
                xor = np.concatenate([stream_bytes(rng, 20 // ib, ib), np.zeros((8 // ib, ib), np.uint8),
                                      stream_bytes(rng, 16 // ib, ib)])
            elif kind in ("malformed", "overlong", "none"):
                vals = rand_inputs(rng, 3 + redo, ib)
            blank = last == -1 or start - 1 == -1
            ref = np.zeros(ib, np.uint8) if blank else rng.integers(0, 256, ib, dtype=np.uint8)
            if not blank:
                raw[(start - 1) & M, h, s] = ref
            if xor is None:
                xor = vals ^ ref[None, :]
            data = O.wire_encode(bytes(ib), xor)  # against a blank reference the stream is the input
            if kind == "malformed":  # a valid first segment, then a header that runs off the packet's end
                data += bytes([0x80]) if s % 2 else bytes([0x0A, 1, 2])
            assert len(data) <= STRIDE, (kind, len(data))
            pk[h, s, :len(data)] = np.frombuffer(data, np.uint8)
            upto[h, s], st[h, s] = last, start
            ln[h, s] = {"overlong": STRIDE + 1 + int(rng.integers(0, 1 << 20)), "none": -5 * (s % 2)}.get(kind, len(data))
    for a in (raw, upto, pk, ln, st):
        a.setflags(write=False)
    return raw, upto, pk, ln, st, kinds


ENCODE_KINDS = ["new", "nothing", "first", "first_none", "fit_R", "over_R", "over_R5", "first_fit", "first_over", "exact",
                "over", "new", "held"]
FIRST_FRAME = 2
EXACT = {1: [("rnd", 31)], 2: [("eq", 2), ("rnd", 15)], 4: [("eq", 1), ("rnd", 3), ("eq", 1), ("rnd", 4)]}


@functools.lru_cache(maxsize=None)
def encode_case(ib, P, mask, seed=0):
    """A sender's ring and one (acked, newest) per endpoint: (raw [R, P, S, ib], acked, newest [P, S],
    kinds).  Frame f of an endpoint is whatever slot f & (R - 1) of its column holds."""
    rng = np.random.default_rng(2000 * ib + 10 * P + mask + seed)
    raw = np.zeros((R, P, S, ib), np.uint8)
    acked = np.full((P, S), SENT, np.int32)
    newest = np.full((P, S), SENT, np.int32)
    kinds = {}
    for h in range(P):
        for s in range(S):
            raw[:, h, s] = rand_inputs(rng, R, ib) if (s + h) % 3 else block_stream(rng, R, ib)
    for h in handles_of(mask, P):
        for s in range(S):
            kind = ENCODE_KINDS[(s + 5 * h) % len(ENCODE_KINDS)]
            kinds[h, s] = kind
            a = int(rng.integers(0, 1 << 30) - R - 8)
            if kind in ("new", "held"):
                nw = a + int(rng.integers(1, 6))
                if kind == "held":
                    raw[:, h, s] = raw[0, h, s]
                    nw = a + int(rng.integers(4, 40))
            elif kind == "nothing":
                nw = a - int(rng.integers(0, 4))
            elif kind == "first":
                a, nw = -1, FIRST_FRAME + int(rng.integers(0, 5))
            elif kind == "first_none":
                a, nw = -1, FIRST_FRAME - 1 - int(rng.integers(0, 3))
            elif kind == "fit_R":
                nw = a + R - 1
            elif kind == "over_R":
                nw = a + R
            elif kind == "over_R5":
                nw = a + R + 5
            elif kind == "first_fit":
                a, nw = -1, FIRST_FRAME + R - 1
            elif kind == "first_over":
                a, nw = -1, FIRST_FRAME + R
            else:  # a packet of exactly TIGHT bytes, or one input more
                spec = EXACT[ib] + ([("rnd", 1)] if kind == "over" else [])
                f = a + 1
                for what, count in spec:
                    x = stream_bytes(rng, count, ib) if what == "rnd" else np.zeros((count, ib), np.uint8)
                    raw[np.arange(f, f + count) & M, h, s] = x ^ raw[a & M, h, s][None, :]
                    f += count
                nw = f - 1
            acked[h, s], newest[h, s] = a, nw
    for x in (raw, acked, newest):
        x.setflags(write=False)
    return raw, acked, newest, kinds


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_header_signatures_and_integration_rows():
    header = open(os.path.join(ROOT, "include", "ggrs_amd.h")).read()
    for name in ("rb_decode_input_packets_all", "rb_encode_input_packets_all"):
        assert re.search(r"^rb_status " + name + r"\(int32_t device, void\* stream, uint32_t handle_mask,", header, re.M)
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = L.load()
    sig = {name: (res, args) for name, res, args in L.SIGNATURES}
    P_, I_, U_, Q_ = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64
    want = {"rb_decode_input_packets_all": [I_, P_, U_, I_, I_, I_, I_, P_, Q_, P_, P_, P_, I_, I_, P_, P_],
            "rb_encode_input_packets_all": [I_, P_, U_, I_, I_, I_, P_, I_, I_, I_, P_, P_, P_, Q_, P_, P_]}
    for name, args in want.items():
        assert sig[name] == (I_, args)
        fn = getattr(lib, name)
        assert fn.restype is I_ and fn.argtypes == args
    assert hasattr(G.DeliveryRing, "receive_packets") and hasattr(G.DeliveryRing, "send_packets")
    assert G.decode_packets is decode_packets and G.encode_packets is encode_packets


def one_pass_shape(data, ib):
    n, h0 = len(data), data[0]
    if not h0 & 0x81 and h0 >> 1 == n - 1 and n <= 32 and (n - 1) % ib == 0:
        return "lit"
    if h0 & 0x81 == 1 and n == 1 and (h0 >> 2) % ib == 0:
        return "run"
    return None


def test_schedules_hold_every_case_the_kernels_can_get_wrong():
    """On the model alone: the counts of every situation, over the schedules the GPU tests run."""
    seen = dict.fromkeys(("wrap", "ref_top", "resent", "first", "stale", "edge_stale", "gap", "malformed_after_valid",
                          "overlong", "cap", "lit", "run", "long", "apart", "old_match", "negative_start"), 0)
    for ib in (1, 2, 4):
        for P, mask in CASES:
            raw0, upto0, pk, ln, st, kinds = decode_case(ib, P, mask)
            raw, upto, status = raw0.copy(), upto0.copy(), np.full((P, S), SENT, np.int32)
            took = model_decode(raw, upto, status, mask, pk, ln, st)
            hs = handles_of(mask, P)
            live = upto0[hs][upto0[hs] >= 0]
            seen["apart"] += int(live.max() - live.min() > R)
            for (h, s), kind in kinds.items():
                last, start, n, code = int(upto0[h, s]), int(st[h, s]), int(ln[h, s]), int(status[h, s])
                data = pk[h, s, :n].tobytes() if 0 < n <= STRIDE else b""
                if (h, s) in took:
                    lo, hi, carried = took[h, s]
                    assert code == 0 and upto[h, s] == hi
                    seen["wrap"] += hi - lo < R and hi & M < lo & M
                    seen["ref_top"] += last != -1 and (start - 1) & M == M and start & M == 0
                    seen["resent"] += start <= last
                    seen["first"] += last == -1 and 0 <= start <= 3
                    seen["negative_start"] += start < 0
                    seen["old_match"] += last == -1 and bool(raw0[:, h, s].any())
                    seen["cap"] += carried > R and hi - lo + 1 == R
                    seen["edge_stale"] += last != -1 and start - 1 == last - 2 * W
                    shape = one_pass_shape(data, ib)
                    seen["lit"] += shape == "lit"
                    seen["run"] += shape == "run"
                    seen["long"] += n > 32
                elif kind == "stale":
                    dec = O.wire_decode(bytes(ib), data)
                    assert code == 1 and start - 1 < last - 2 * W and start + len(dec) - 1 > last
                    seen["stale"] += 1
                elif code == -2:
                    seen["gap"] += 1
                elif code == -1 and n > STRIDE:
                    seen["overlong"] += 1
                elif code == -1:
                    first = segments_prefix(data)
                    assert O.wire_decode(bytes(ib), data[:first]) is not None and O.wire_decode(bytes(ib), data) is None
                    seen["malformed_after_valid"] += 1
                elif kind == "neg_ref":
                    assert code == 1 and start < 0
                    seen["negative_start"] += 1
            for h in range(P):  # rows outside the mask are nobody's
                if h not in hs:
                    assert (status[h] == SENT).all() and (upto[h] == SENT).all()
                    np.testing.assert_array_equal(raw[:, h], raw0[:, h])
    assert all(v >= 1 for v in seen.values()), seen
    enc = dict.fromkeys(("nothing", "too_long", "overrun", "exactly_R", "first_exactly_R", "fits_exactly", "over_by_little",
                         "first"), 0)
    for ib in (1, 2, 4):
        for P, mask in CASES:
            raw, acked, newest, kinds = encode_case(ib, P, mask)
            roomy = model_encode(raw, mask, acked, newest, FIRST_FRAME, ROOMY)
            tight = model_encode(raw, mask, acked, newest, FIRST_FRAME, TIGHT)
            assert (roomy[1] != -1).all() and (roomy[2] == tight[2]).all()
            for (h, s), kind in kinds.items():
                a, nw, n, nt = int(acked[h, s]), int(newest[h, s]), int(roomy[1][h, s]), int(tight[1][h, s])
                enc["nothing"] += n == 0
                enc["overrun"] += n == -2 and nt == -2
                enc["too_long"] += nt == -1 and n > TIGHT
                enc["exactly_R"] += n > 0 and a != -1 and nw - a + 1 == R
                enc["first_exactly_R"] += n > 0 and a == -1 and nw - FIRST_FRAME + 1 == R
                enc["first"] += n > 0 and a == -1
                enc["fits_exactly"] += n == TIGHT and nt == TIGHT
                enc["over_by_little"] += TIGHT < n <= TIGHT + 4 and nt == -1
                if kind in ("over_R", "over_R5", "first_over"):
                    assert n == -2
    assert all(v >= 1 for v in enc.values()), enc


def segments_prefix(data):
    """The length of a packet's first segment (its header is whole and its literal fits)."""
    v, sh, p = 0, 0, 0
    while True:
        b = data[p]
        p += 1
        v |= (b & 0x7F) << sh
        sh += 7
        if not b & 0x80:
            break
    return p if v & 1 else p + (v >> 1)


# ---------------------------------------------------------------------------
# the device calls: numpy in, numpy out, every tensor between guard regions
# ---------------------------------------------------------------------------
GUARD = 256


class Guarded:
    """A device tensor of `array`'s bytes between two guard regions of a pattern."""

    def __init__(self, array):
        import torch
        self.array = np.ascontiguousarray(array)
        n = self.array.nbytes
        self.flat = torch.empty(2 * GUARD + n, dtype=torch.uint8, device="cuda")
        self.pattern = torch.arange(GUARD, dtype=torch.int32, device="cuda").mul(37).add(11).to(torch.uint8)
        self.flat[:GUARD] = self.pattern
        self.flat[GUARD + n:] = self.pattern
        self.flat[GUARD:GUARD + n] = torch.from_numpy(self.array.view(np.uint8).reshape(-1)).cuda()
        self.n = n

    def ptr(self, offset=0):
        return ctypes.c_void_p(self.flat.data_ptr() + GUARD + offset)

    def read(self):
        """The tensor's content now; asserts both guards unchanged."""
        host = self.flat.cpu().numpy()
        pat = self.pattern.cpu().numpy()
        assert (host[:GUARD] == pat).all() and (host[GUARD + self.n:] == pat).all(), "a guard region was written"
        return host[GUARD:GUARD + self.n].view(self.array.dtype).reshape(self.array.shape).copy()


def call_decode(raw, upto, status, mask, pk, ln, st, max_prediction=W, ring_frames=R, per_handle=False):
    """rb_decode_input_packets_all on copies of the arrays (per_handle: rb_decode_input_packets once
    per handle of the mask): (rb_status, raw, upto, status)."""
    import torch
    lib = L.load()
    F, P, n, ib = raw.shape
    stride = pk.shape[2]
    g = [Guarded(a) for a in (raw, upto, status, pk, ln, st)]
    graw, gupto, gstatus, gpk, gln, gst = g
    if per_handle:
        rc = 0
        for h in handles_of(mask, P):
            rc |= lib.rb_decode_input_packets(0, None, h, P, n, ib, max_prediction, gpk.ptr(h * n * stride), stride,
                                              gln.ptr(4 * h * n), gst.ptr(4 * h * n), graw.ptr(), F, gupto.ptr(),
                                              gstatus.ptr(4 * h * n))
    else:
        rc = lib.rb_decode_input_packets_all(0, None, mask, P, n, ib, max_prediction, gpk.ptr(), stride, gln.ptr(),
                                             gst.ptr(), graw.ptr(), F, ring_frames, gupto.ptr(), gstatus.ptr())
    torch.cuda.synchronize()
    out = [x.read() for x in g]
    for before, after in zip((pk, ln, st), out[3:]):
        np.testing.assert_array_equal(after, before, err_msg="decode wrote one of its inputs")
    return rc, out[0], out[1], out[2]


def call_encode(raw, mask, acked, newest, first_frame, stride, ring_frames=R, per_handle=False, fill=0xEE):
    """rb_encode_input_packets_all on copies (per_handle: rb_encode_input_packets per handle):
    (rb_status, pk [P, S, stride], ln, st); rows nobody writes keep `fill` / SENT."""
    import torch
    lib = L.load()
    F, P, n, ib = raw.shape
    g = [Guarded(a) for a in (raw, acked, newest, np.full((P, n, stride), fill, np.uint8), np.full((P, n), SENT, np.int32),
                              np.full((P, n), SENT, np.int32))]
    graw, gack, gnew, gpk, gln, gst = g
    if per_handle:
        rc = 0
        for h in handles_of(mask, P):
            rc |= lib.rb_encode_input_packets(0, None, h, P, n, ib, graw.ptr(), F, first_frame, gack.ptr(4 * h * n),
                                              gnew.ptr(4 * h * n), gpk.ptr(h * n * stride), stride, gln.ptr(4 * h * n),
                                              gst.ptr(4 * h * n))
    else:
        rc = lib.rb_encode_input_packets_all(0, None, mask, P, n, ib, graw.ptr(), F, ring_frames, first_frame, gack.ptr(),
                                             gnew.ptr(), gpk.ptr(), stride, gln.ptr(), gst.ptr())
    torch.cuda.synchronize()
    out = [x.read() for x in g]
    for before, after in zip((raw, acked, newest), out[:3]):
        np.testing.assert_array_equal(after, before, err_msg="encode wrote one of its inputs")
    return rc, out[3], out[4], out[5]


def assert_packets(pk, ln, st, want, what, fill=0xEE):
    """Lengths, start frames and the packets' bytes against model_encode's; rows the call does not
    own keep their fill.  Bytes past a packet's length are unspecified."""
    packets, wln, wst = want
    np.testing.assert_array_equal(ln, wln, err_msg=f"lengths, {what}")
    np.testing.assert_array_equal(st, wst, err_msg=f"start frames, {what}")
    for h in range(pk.shape[0]):
        for s in range(pk.shape[1]):
            if wln[h, s] == SENT:
                assert (pk[h, s] == fill).all(), f"{what}: a row outside the mask was written ({h}, {s})"
            elif wln[h, s] == -2:
                assert (pk[h, s] == fill).all(), f"{what}: an overrun endpoint's row was written ({h}, {s})"
            elif wln[h, s] > 0:
                assert pk[h, s, :wln[h, s]].tobytes() == packets[h, s], f"{what}: packet ({h}, {s})"


# ---------------------------------------------------------------------------
# GPU 1: ring decode against the model
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P,mask", CASES)
@pytest.mark.parametrize("ib", [1, 2, 4])
def test_gpu_ring_decode_matches_the_model(gpu_available, ib, P, mask):
    raw0, upto0, pk, ln, st, _ = decode_case(ib, P, mask)
    want_raw, want_upto, want_status = raw0.copy(), upto0.copy(), np.full((P, S), SENT, np.int32)
    model_decode(want_raw, want_upto, want_status, mask, pk, ln, st)
    rc, raw, upto, status = call_decode(raw0, upto0, np.full((P, S), SENT, np.int32), mask, pk, ln, st)
    assert rc == L.RB_OK
    np.testing.assert_array_equal(status, want_status, err_msg="status")
    np.testing.assert_array_equal(upto, want_upto, err_msg="upto")
    np.testing.assert_array_equal(raw, want_raw, err_msg="the ring: written slots, and every slot not written")
    assert {0, 1, -1, -2, SENT} == set(np.unique(status).tolist())


# ---------------------------------------------------------------------------
# GPU 2: linear mode equals the existing entry points
# ---------------------------------------------------------------------------
def linear_decode_case(ib, P, mask):
    """The vector table of test_wire_edges under its three receiver states, then random lanes in the
    style of test_wire's decode test (re-sent frames, truncated packets, gaps, negative start frames,
    references at and past the tensor's end, packets that run past it)."""
    rows = [r for r in TABLE if r[1] == ib]
    V, RF = len(rows), 40
    states = [(-1, 0), (11, 10), (RF - 3, RF - 2)]
    assert 3 * V <= S and max(len(r[3]) for r in rows) <= STRIDE
    rng = np.random.default_rng(300 + ib + mask)
    raw = rng.integers(0, 256, (RF, P, S, ib), dtype=np.uint8)
    pk = np.zeros((P, S, STRIDE), np.uint8)
    ln, st = np.zeros((P, S), np.int32), np.zeros((P, S), np.int32)
    upto = np.full((P, S), SENT, np.int32)
    for h in handles_of(mask, P):
        for s in range(S):
            if s < 3 * V:
                last, start = states[s // V]
                _, _, ref, data, _ = rows[s % V]
            else:
                last = int(rng.integers(-1, RF + 2))
                start = last + 1 - int(rng.integers(0, 3)) if last >= 2 else int(rng.integers(0, 3))
                vals = rand_inputs(rng, int(rng.integers(1, 9)), ib)
                ref = rng.integers(0, 256, ib, dtype=np.uint8).tobytes()
                data = O.wire_encode(bytes(ib) if last == -1 or start == 0 else ref, vals)
                pick = rng.random()
                if pick < 0.08:
                    data = data[:-1] + bytes([data[-1] | 0x80])
                elif pick < 0.16:
                    start = last + 2
                elif pick < 0.24:
                    start, last = -3, min(max(last, 0), 4)
                elif pick < 0.30:
                    start = RF + int(rng.integers(0, 3))  # the reference at / past the tensor's end
                    last = start - 1 + int(rng.integers(0, 2))
            if last != -1 and 1 <= start <= RF:
                raw[start - 1, h, s] = np.frombuffer(ref, np.uint8)
            pk[h, s, :len(data)] = np.frombuffer(data, np.uint8)
            ln[h, s], st[h, s], upto[h, s] = len(data), start, last
        ln[h, S - 1], ln[h, S - 2] = STRIDE + 1, 0
    return raw, upto, pk, ln, st


@pytest.mark.gpu
@pytest.mark.parametrize("P,mask", CASES)
@pytest.mark.parametrize("ib", [1, 2, 4])
def test_gpu_linear_decode_equals_the_per_handle_entry_point(gpu_available, ib, P, mask):
    raw0, upto0, pk, ln, st = linear_decode_case(ib, P, mask)
    status0 = np.full((P, S), SENT, np.int32)
    old = call_decode(raw0, upto0, status0, mask, pk, ln, st, per_handle=True)
    new = call_decode(raw0, upto0, status0, mask, pk, ln, st, ring_frames=0)
    assert old[0] == new[0] == L.RB_OK
    for a, b, name in zip(old[1:], new[1:], ("inputs", "upto", "status")):
        np.testing.assert_array_equal(b, a, err_msg=name)
    codes = set(np.unique(new[3]).tolist())
    assert {0, 1, -1, -2, SENT} == codes
    assert (new[1] != raw0).any() and (new[2] != upto0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("ib", [1, 2, 4])
def test_gpu_linear_encode_equals_the_per_handle_entry_point(gpu_available, ib):
    P, mask, F = 4, 0b1101, 160
    rng = np.random.default_rng(50 + ib)
    raw = np.zeros((F, P, S, ib), np.uint8)
    for h in range(P):
        for s in range(S):
            raw[:, h, s] = block_stream(rng, F, ib) if s % 2 else rand_inputs(rng, F, ib)
    acked = rng.integers(-1, 50, (P, S)).astype(np.int32)
    newest = (acked + rng.integers(-2, 101, (P, S))).astype(np.int32)
    newest[:, ::17] += 200  # at and past the tensor's end: nothing is sent
    seen = set()
    for stride in (ROOMY, TIGHT, 48):
        for first in (0, 3):
            old = call_encode(raw, mask, acked, newest, first, stride, per_handle=True)
            new = call_encode(raw, mask, acked, newest, first, stride, ring_frames=0)
            assert old[0] == new[0] == L.RB_OK
            np.testing.assert_array_equal(new[2], old[2], err_msg=f"lengths, stride {stride}")
            np.testing.assert_array_equal(new[3], old[3], err_msg=f"start frames, stride {stride}")
            for h, s in zip(*np.nonzero(old[2] > 0)):
                assert new[1][h, s, :old[2][h, s]].tobytes() == old[1][h, s, :old[2][h, s]].tobytes(), (stride, h, s)
            assert (new[1][1] == 0xEE).all() and (new[2][1] == SENT).all()
            seen |= set(np.unique(np.sign(new[2][[0, 2, 3]])).tolist())
            assert int(new[2].max()) > 32 or stride == TIGHT
    assert seen == {0, 1, -1}


# ---------------------------------------------------------------------------
# GPU 3: ring encode against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P,mask", CASES)
@pytest.mark.parametrize("ib", [1, 2, 4])
def test_gpu_ring_encode_matches_the_oracle(gpu_available, ib, P, mask):
    raw, acked, newest, _ = encode_case(ib, P, mask)
    for stride in (ROOMY, TIGHT):
        want = model_encode(raw, mask, acked, newest, FIRST_FRAME, stride)
        rc, pk, ln, st = call_encode(raw, mask, acked, newest, FIRST_FRAME, stride)
        assert rc == L.RB_OK
        assert_packets(pk, ln, st, want, f"stride {stride}")
        assert ({0, -2} <= set(np.unique(ln).tolist())) and ((ln == -1).any() == (stride == TIGHT))


# ---------------------------------------------------------------------------
# GPU 4: round trip
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ib", [1, 2, 4])
def test_gpu_ring_round_trip_between_sessions_far_apart(gpu_available, ib):
    """Ring encode -> ring decode on a receiver that already holds the frames up to a random `last`
    in [acked, min(newest, acked + 2 W)]: its slots of frames last + 1 .. newest end up the sender's, its other slots
    stay, upto is newest."""
    P, mask = 4, 0b0110
    rng = np.random.default_rng(70 + ib)
    send = rng.integers(0, 256, (R, P, S, ib), dtype=np.uint8)
    for s in range(0, S, 2):
        send[:, 1, s] = rand_inputs(rng, R, ib)
    acked = (rng.integers(0, 1 << 30, (P, S)) - R).astype(np.int32)
    acked[:, ::9] = -1
    newest = np.where(acked == -1, FIRST_FRAME, acked + 1).astype(np.int32) + rng.integers(0, 90, (P, S)).astype(np.int32)
    assert acked[1].max() - acked[1][acked[1] >= 0].min() > R
    rc, pk, ln, st = call_encode(send, mask, acked, newest, FIRST_FRAME, ROOMY)
    assert rc == L.RB_OK and (ln[[1, 2]] > 0).all() and (ln[[1, 2]] > 32).any()
    # (no further: a packet whose reference is more than 2 W frames behind `last` is ignored)
    ahead = rng.integers(0, 1 << 20, (P, S)) % np.minimum(newest - acked + 1, 2 * W + 1)
    last = np.where(acked == -1, -1, acked + ahead).astype(np.int32)
    recv = rng.integers(0, 256, (R, P, S, ib), dtype=np.uint8)
    cols = np.arange(S)
    for h in (1, 2):
        recv[acked[h] & M, h, cols] = send[acked[h] & M, h, cols]  # the reference input: a frame the receiver has
    want = recv.copy()
    for h in (1, 2):
        for s in range(S):
            f = np.arange(max(last[h, s] + 1, st[h, s]), newest[h, s] + 1)  # (a first packet starts at the sender's delay)
            want[f & M, h, s] = send[f & M, h, s]
    status0 = np.full((P, S), SENT, np.int32)
    ln, st = np.where(ln == SENT, 0, ln), np.where(st == SENT, 0, st)
    rc, got, upto, status = call_decode(recv, last, status0, mask, pk, ln, st)
    assert rc == L.RB_OK
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(upto[[1, 2]], newest[[1, 2]])
    np.testing.assert_array_equal(upto[[0, 3]], last[[0, 3]])
    np.testing.assert_array_equal(status[[1, 2]], np.where(newest > last, 0, 1)[[1, 2]])
    assert (status[[1, 2]] == 1).any() and (status[[0, 3]] == SENT).all()


# ---------------------------------------------------------------------------
# GPU 7: validation
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_invalid_requests_touch_nothing(gpu_available):
    import torch
    lib = L.load()
    ib, P, mask = 1, 4, 0b0110
    raw0, upto0, pk, ln, st, _ = decode_case(ib, 4, 0b1110)
    status0 = np.full((P, S), SENT, np.int32)
    big = np.concatenate([raw0, raw0])  # a tensor of 2R frames
    bad_decode = [  # (what, keyword changes)
        ("empty mask", dict(mask=0)), ("a bit at num_players", dict(mask=0b10000)),
        ("stride 40", dict(pk=np.ascontiguousarray(pk[:, :, :40]))), ("stride 16", dict(pk=np.ascontiguousarray(pk[:, :, :16]))),
        ("ring of 96", dict(raw=raw0[:96], ring_frames=96)), ("ring of 64", dict(raw=raw0[:64], ring_frames=64)),
        ("frames != ring", dict(raw=big, ring_frames=R)), ("2W == R", dict(max_prediction=R // 2)),
        ("W == 0", dict(max_prediction=0)),
    ]
    for what, kw in bad_decode:
        a = dict(raw=raw0, upto=upto0, status=status0, mask=mask, pk=pk, ln=ln, st=st, max_prediction=W, ring_frames=R)
        a.update(kw)
        rc, raw, upto, status = call_decode(**a)
        assert rc == L.RB_INVALID_REQUEST, what
        np.testing.assert_array_equal(raw, a["raw"], err_msg=what)
        np.testing.assert_array_equal(upto, upto0, err_msg=what)
        np.testing.assert_array_equal(status, status0, err_msg=what)
    rc, _, _, status = call_decode(raw0, upto0, status0, mask, pk, ln, st, max_prediction=R // 2 - 1)
    assert rc == L.RB_OK and (status[[1, 2]] != SENT).all()  # the largest window a ring of R serves
    eraw, acked, newest, _ = encode_case(ib, 4, 0b1110)
    bad_encode = [("empty mask", dict(mask=0)), ("a bit at num_players", dict(mask=0b110000)), ("stride 40", dict(stride=40)),
                  ("stride 16", dict(stride=16)), ("ring of 96", dict(raw=eraw[:96], ring_frames=96)),
                  ("ring of 100", dict(raw=eraw[:100], ring_frames=100)), ("frames != ring", dict(raw=np.concatenate([eraw, eraw])))]
    for what, kw in bad_encode:
        a = dict(raw=eraw, mask=mask, acked=acked, newest=newest, first_frame=FIRST_FRAME, stride=ROOMY, ring_frames=R)
        a.update(kw)
        rc, epk, eln, est = call_encode(**a)
        assert rc == L.RB_INVALID_REQUEST, what
        assert (epk == 0xEE).all() and (eln == SENT).all() and (est == SENT).all(), what
    # the arguments numpy shapes cannot carry: five players, input sizes, alignment
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in
         dict(raw=raw0, upto=upto0, status=status0, pk=pk, ln=ln, st=st, acked=acked, newest=newest).items()}
    keep = {k: v.clone() for k, v in t.items()}
    p = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)

    def dec(mask=mask, P=P, ib=1, off=0):
        return lib.rb_decode_input_packets_all(0, None, mask, P, S, ib, W, p(t["pk"], off), STRIDE, p(t["ln"]), p(t["st"]),
                                               p(t["raw"]), R, R, p(t["upto"]), p(t["status"]))

    def enc(mask=mask, P=P, ib=1, off=0):
        return lib.rb_encode_input_packets_all(0, None, mask, P, S, ib, p(t["raw"]), R, R, FIRST_FRAME, p(t["acked"]),
                                               p(t["newest"]), p(t["pk"], off), STRIDE, p(t["ln"]), p(t["st"]))

    for fn in (dec, enc):
        assert fn(mask=0b10001, P=5) == L.RB_INVALID_REQUEST and fn(mask=1, P=5) == L.RB_INVALID_REQUEST
        for size in (0, 3, 8):
            assert fn(ib=size) == L.RB_INVALID_REQUEST
        assert fn(off=8) == L.RB_INVALID_REQUEST and fn(off=4) == L.RB_INVALID_REQUEST
    torch.cuda.synchronize()
    for k in t:
        assert torch.equal(t[k], keep[k]), k
    ring = G.DeliveryRing(R, P, S)
    with pytest.raises(G.InvalidRequest):
        ring.receive_packets(0, t["pk"], t["ln"], t["st"], W)
    with pytest.raises(G.InvalidRequest):
        ring.send_packets(0b10000, t["newest"], t["acked"], 0, t["pk"], t["ln"], t["st"])
    assert (ring.upto == G.NULL_FRAME).all() and not ring.inputs.any()


# ---------------------------------------------------------------------------
# GPU 5: closed loops over bytes only
# ---------------------------------------------------------------------------
LOOP_T, LOOP_RESTART, LOOP_STRIDE, LOOP_D = 300, 140, 128, 0
EPOCH, FPS = 12, 60


def loop_lag(n=SL):
    return 1 + np.arange(n) % 4          # ticks an ack takes to come back, per session


def loop_drops(n=SL, links=2):
    """[LOOP_T, links, n] bool: the seeded tenth of the packets that never arrive."""
    return np.random.default_rng(SEED & 0xFFFF).random((LOOP_T, links, n)) < 0.1


class Link:
    """The sender's state of the endpoints of `mask` (its `sent`, the acks as they came back, the
    packets of this tick), on the device and in the model."""

    def __init__(self, P, mask, n, ib):
        import torch
        self.P, self.mask, self.n, self.ib = P, mask, n, ib
        self.pk = torch.zeros((P, n, LOOP_STRIDE), dtype=torch.uint8, device="cuda")
        self.ln = torch.zeros((P, n), dtype=torch.int32, device="cuda")
        self.st = torch.zeros((P, n), dtype=torch.int32, device="cuda")
        self.status = torch.full((P, n), SENT, dtype=torch.int32, device="cuda")
        self.sent = torch.full((P, n), G.NULL_FRAME, dtype=torch.int32, device="cuda")
        self.hist = [torch.full((P, n), G.NULL_FRAME, dtype=torch.int32, device="cuda") for _ in range(5)]
        self.m_sent = np.full((P, n), -1, np.int32)
        self.m_hist = [np.full((P, n), -1, np.int32) for _ in range(5)]
        self.lag = loop_lag(n)
        self.cols = np.arange(n)

    def acked(self):
        """(device, model): the receiver's watermark as its receive_packets of `lag` ticks ago left it."""
        import torch
        lag = torch.from_numpy(self.lag.astype(np.int64)).cuda()
        cols = torch.from_numpy(self.cols).cuda()
        dev_ = torch.stack(self.hist)[5 - lag, :, cols].t().contiguous()
        mod = np.stack(self.m_hist)[5 - self.lag, :, self.cols].T.copy()
        return dev_, mod

    def push(self, upto, m_upto):
        self.hist = self.hist[1:] + [upto.clone()]
        self.m_hist = self.m_hist[1:] + [m_upto.copy()]

    def restart(self, who):
        import torch
        sel = torch.from_numpy(who).cuda()
        for x in [self.sent] + self.hist:
            x[:, sel] = G.NULL_FRAME
        for x in [self.m_sent] + self.m_hist:
            x[:, who] = -1


def send_and_receive(link, src_ring, m_src, dst_ring, m_dst, m_dst_upto, drop, what):
    """One tick of one link, on the device and in the model, compared: the sender's send_packets out
    of its ring, the seeded drops, the receiver's receive_packets into its ring."""
    import torch
    acked, m_acked = link.acked()
    src_ring.send_packets(link.mask, link.sent, acked, LOOP_D, link.pk, link.ln, link.st)
    want = model_encode(m_src, link.mask, m_acked, link.m_sent, LOOP_D, LOOP_STRIDE)
    assert (want[1] != -1).all() and (want[1] != -2).all(), what
    pk, ln, st = (x.cpu().numpy() for x in (link.pk, link.ln, link.st))
    hs = handles_of(link.mask, link.P)
    np.testing.assert_array_equal(ln[hs], want[1][hs], err_msg=f"lengths, {what}")
    np.testing.assert_array_equal(st[hs], want[2][hs], err_msg=f"start frames, {what}")
    for (h, s), data in want[0].items():
        assert pk[h, s, :len(data)].tobytes() == data, f"packet ({h}, {s}), {what}"
    lost = np.zeros((link.P, link.n), bool)
    lost[hs] = drop
    link.ln[torch.from_numpy(lost).cuda()] = 0
    m_ln = np.where(lost, 0, want[1])
    dst_ring.receive_packets(link.mask, link.pk, link.ln, link.st, W, status=link.status)
    m_pk = np.zeros((link.P, link.n, LOOP_STRIDE), np.uint8)
    for (h, s), data in want[0].items():
        m_pk[h, s, :len(data)] = np.frombuffer(data, np.uint8)
    m_status = np.full((link.P, link.n), SENT, np.int32)
    before = m_dst_upto.copy()
    model_decode(m_dst, m_dst_upto, m_status, link.mask, m_pk, m_ln, want[2])
    np.testing.assert_array_equal(link.status.cpu().numpy()[hs], m_status[hs], err_msg=f"decode status, {what}")
    np.testing.assert_array_equal(dst_ring.upto.cpu().numpy()[hs], m_dst_upto[hs], err_msg=f"upto, {what}")
    assert (m_status[hs] >= 0).all(), what
    link.push(dst_ring.upto, m_dst_upto)
    return int((want[1][hs] > 0).sum()), int(((m_ln[hs] > 0) & (want[2][hs] <= before[hs])).sum())  # (packets, packets with re-sent frames)


class Side:
    """One batch of a closed loop with everything that stands beside it: its DeliveryRing (own
    handles' rows filled by export_local_inputs, the others' by receive_packets), the twin fed the
    model's watermarks and the true inputs directly, the oracles, and the model's ring."""

    def __init__(self, game, P, mask, n, dtype, stream, time_sync=False, desync=0):
        import torch
        from test_delivery_ring import Groups
        from test_time_sync import BatchModel, make_session
        self.P, self.mask, self.n = P, mask, n
        self.ib = np.dtype(dtype).itemsize
        tdt = torch.uint8 if self.ib == 1 else torch.int32
        self.sess, self.twin = (make_session(game, P, mask, LOOP_D, LOOP_D, sessions=n, time_sync=time_sync, desync=desync)
                                for _ in range(2))
        for b in (self.sess, self.twin):
            b.set_stream(stream)
            b.set_delivery_ring(R)
        self.ring = G.DeliveryRing(R, P, n, dtype=tdt)
        self.twin_ring = np.zeros((R, P, n), dtype)
        self.twin_dev = torch.zeros((R, P, n), dtype=tdt, device="cuda")
        self.cls = Groups(game, P, LOOP_D, LOOP_D, mask, n, desync=desync)
        self.model = BatchModel(n, P, mask, LOOP_D, FPS) if time_sync else None
        self.m_ring = np.zeros((R, P, n, self.ib), np.uint8)
        self.m_upto = np.full((P, n), -1, np.int32)
        self.fed = np.full((P, n), -1, np.int64)            # the twin's ring holds the truth up to here
        self.truth = np.zeros((LOOP_T + 8, P, n), dtype)    # every handle's input by frame, as the oracles queued it
        self.uptos = np.full((LOOP_T, P, n), -1, np.int32)
        self.time_sync = time_sync

    def restart(self, who, cohorts):
        from test_time_sync import SessionModel
        for b in (self.sess, self.twin):
            b.restart_sessions(who)
        self.cls.restart(cohorts)
        self.ring.restart(who)
        self.m_upto[:, who] = -1
        self.fed[:, who] = -1
        if self.model is not None:
            for s in np.nonzero(who)[0]:
                self.model.sessions[s] = SessionModel(self.P, self.mask, LOOP_D, FPS)

    def tick(self, t, local, d_local, truth_of, what):
        """Tick t on the batch (fed its ring and the watermarks receive_packets left), on the twin
        and on the oracles (both fed the model's watermarks and the true inputs); everything compared."""
        import torch
        from test_delivery_ring import equal_everything
        from test_p2p_pacing import compare_all
        from test_restart import ALL
        from test_time_sync import assert_same, gpu_state
        cols = np.arange(self.n)
        for h in range(self.P):
            if (self.mask >> h) & 1:
                continue
            self.truth[:, h] = truth_of(h)
            for k in range(int((self.m_upto[h] - self.fed[h]).max())):
                sel = self.fed[h] + 1 + k <= self.m_upto[h]
                f = (self.fed[h] + 1 + k)[sel]
                self.twin_ring[f & M, h, cols[sel]] = self.truth[f, h, cols[sel]]
            self.fed[h] = np.maximum(self.fed[h], self.m_upto[h])
        self.twin_dev.copy_(torch.from_numpy(self.twin_ring.view(np.int32) if self.ib == 4 else self.twin_ring))
        self.uptos[t] = self.m_upto
        self.sess.run_ticks(d_local[t:t + 1], self.ring.upto[None].clone(), self.ring.inputs)
        self.twin.run_ticks(d_local[t:t + 1], torch.from_numpy(self.m_upto.copy()).cuda()[None], self.twin_dev)
        cur = self.cls.frames()[0] if self.model is not None else None
        before = self.cls.queues()[:, :, 6].copy()
        self.cls.tick(t, ALL, local, self.uptos, self.truth.copy())
        after = self.cls.queues()[:, :, 6]
        for h in range(self.P):  # what add_local_input queued this tick: the frame's true input
            if (self.mask >> h) & 1:
                added = after[:, h] > before[:, h]
                self.truth[after[added, h], h, cols[added]] = local[t, h, cols[added]]
        if self.model is not None:
            nobody = np.zeros((self.n, self.P), bool)
            self.model.tick(cur, self.cls.st, nobody, nobody, self.m_upto)
        compare_all(self.sess, self.cls, what)
        equal_everything(self.sess, self.twin, self.time_sync, what)
        if self.model is not None:
            assert_same(gpu_state(self.sess), self.model.state(), f"time sync against the model, {what}")

    def exported(self, link, what):
        """export_local_inputs into the side's own ring; the model's ring and `sent` from the oracles' queues."""
        self.sess.export_local_inputs(self.ring.inputs, link.sent)
        last = self.cls.queues()[:, :, 6]
        cols = np.arange(self.n)
        for h in handles_of(self.mask, self.P):
            new = np.maximum(last[:, h], -1).astype(np.int64)
            old = link.m_sent[h].astype(np.int64)
            for k in range(int((new - old).max())):
                sel = old + 1 + k <= new
                f = (old + 1 + k)[sel]
                self.m_ring[f & M, h, cols[sel]] = self.truth[f, h, cols[sel]][:, None].view(np.uint8)
            link.m_sent[h] = new
        np.testing.assert_array_equal(link.sent.cpu().numpy()[handles_of(self.mask, self.P)],
                                      link.m_sent[handles_of(self.mask, self.P)], err_msg=f"sent, {what}")

    def close(self):
        for b in (self.sess, self.twin, self.cls):
            b.close()


LOOPS = {  # name: game, input dtype, input mask, time sync, desync interval
    "exgame": (G.Game.EX_GAME, np.uint8, 0x0F, False, 0),
    "exgame-time-sync-desync": (G.Game.EX_GAME, np.uint8, 0x0F, True, 10),
    "stub-u32": (G.Game.STUB, np.uint32, 0xFFFFFFFF, False, 0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LOOPS))
def test_gpu_two_batches_play_each_other_over_bytes_only(gpu_available, name):
    """Side A (handle 0 local) and side B (handle 1 local): per tick each exports its local inputs
    into its ring, encodes them against the ack that came back 1-4 ticks late, a tenth of the packets
    is lost, the peer decodes the rest into its ring and runs its tick on the resulting watermarks.
    Every third pair restarts after 140 ticks.  After every tick each batch equals the oracles and a
    twin, both fed the model's watermarks and the true inputs."""
    import torch
    from test_p2p_pacing import dev
    from test_restart import cohort_mask, cohort_of
    from test_time_sync import quality
    game, dtype, imask, time_sync, desync = LOOPS[name]
    X = G.synth_inputs(SL, 2, LOOP_T, seed=SEED ^ 0x100F, mask=imask, dtype=dtype)
    drops = loop_drops()
    stream = torch.cuda.Stream()
    sent_packets = resent = 0
    with torch.cuda.stream(stream):
        sides = [Side(game, 2, m, SL, dtype, stream, time_sync, desync) for m in (0b01, 0b10)]
        links = [Link(2, m, SL, np.dtype(dtype).itemsize) for m in (0b01, 0b10)]
        dx = dev(X.view(np.int32) if dtype == np.uint32 else X)
        who = cohort_mask(SL, (1,)) != 0
        for t in range(LOOP_T):
            if t == LOOP_RESTART:
                for side, link in zip(sides, links):
                    side.restart(who, (1,))
                    link.restart(who)
            if time_sync and t % EPOCH == 0:
                for side in sides:
                    h = 1 if side.mask == 0b01 else 0
                    rtt, adv = quality(t // EPOCH, h, SL)
                    for b in (side.sess, side.twin):
                        b.receive_quality(h, *dev(rtt, adv))
                    side.model.receive_quality(h, rtt, adv)
            for i, (side, link) in enumerate(zip(sides, links)):
                peer = sides[1 - i]
                side.exported(link, f"side {'AB'[i]}, tick {t}")
                a, b = send_and_receive(link, side.ring, side.m_ring, peer.ring, peer.m_ring, peer.m_upto, drops[t, i],
                                        f"link {'AB'[i]} -> {'BA'[i]}, tick {t}")
                sent_packets, resent = sent_packets + a, resent + b
            for i, side in enumerate(sides):
                peer = sides[1 - i]
                side.tick(t, X, dx, lambda h: peer.truth[:, h], f"side {'AB'[i]}, tick {t}")
        cur, co = sides[0].sess.frames()[0], cohort_of(SL)
        assert (cur[co != 1] > 2 * R).all() and (cur[co == 1] < cur[co != 1].min() - R + 20).all(), "the rings wrapped twice"
        assert resent > SL and sent_packets > LOOP_T * SL
        assert all((s.cls.lf >= 0).any() for s in sides) and all(s.sess.counters()[2] == 0 for s in sides)
        for s in sides:
            s.close()


def synthetic_sender(P, mask, ticks, n=SL):
    """A schedule of test_p2p's network for a batch whose local handles are `mask`: (local inputs,
    the newest frame each remote peer has produced per tick [T, P, n], the peers' inputs by frame)."""
    return synth_network(n, P, ticks, mask, 1, 1, 4, seed=SEED ^ 0x5E7D)


@pytest.mark.gpu
@pytest.mark.parametrize("P,mask,k", [(4, 0b0001, 1), (2, 0b01, 7)], ids=["p4-one-tick", "p2-seven-ticks"])
def test_gpu_batch_fed_by_a_synthetic_sender_over_bytes(gpu_available, P, mask, k):
    """ex_game with every remote handle's packets encoded in one launch out of a sender ring and
    decoded in one launch into the batch's ring (P = 4: three endpoints per session; a four-sided
    mesh of batches would run this file's loop four times over for the same codec calls).  k = 7:
    the deliveries of a call's 7 ticks are decoded before the call, one watermark row per tick.
    Late acks, lost packets and the comparisons are the closed loop's; the sender's ring is filled
    with torch from the schedule."""
    import torch
    from test_delivery_ring import equal_everything
    from test_p2p_pacing import compare_all, dev
    from test_restart import ALL, Cohorts
    from test_time_sync import make_session
    rmask = ((1 << P) - 1) & ~mask
    remotes = handles_of(rmask, P)
    inputs, newest, rin = synthetic_sender(P, mask, LOOP_T)
    drops = loop_drops(SL, len(remotes))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        sess, twin = (make_session(G.Game.EX_GAME, P, mask, 1, 1, sessions=SL, time_sync=False) for _ in range(2))
        for b in (sess, twin):
            b.set_stream(stream)
            b.set_delivery_ring(R)
        cls = Cohorts(G.Game.EX_GAME, P, 1, 1, mask, SL)
        link = Link(P, rmask, SL, 1)
        sender, ring = G.DeliveryRing(R, P, SL), G.DeliveryRing(R, P, SL)
        m_sender, m_ring = np.zeros((R, P, SL, 1), np.uint8), np.zeros((R, P, SL, 1), np.uint8)
        m_upto = np.full((P, SL), -1, np.int32)
        twin_ring, fed = np.zeros((R, P, SL), np.uint8), np.full((P, SL), -1, np.int64)
        uptos = np.full((LOOP_T, P, SL), -1, np.int32)
        di = dev(inputs)
        cols = np.arange(SL)
        resent = 0
        for t0 in range(0, LOOP_T, k):
            t1 = min(t0 + k, LOOP_T)
            rows = []
            for t in range(t0, t1):
                for h in remotes:  # the peers' new frames into the sender's ring: frame f in slot f & (R - 1)
                    old, new = link.m_sent[h].astype(np.int64), newest[t, h].astype(np.int64)
                    for j in range(int((new - old).max())):
                        sel = old + 1 + j <= new
                        f = (old + 1 + j)[sel]
                        m_sender[f & M, h, cols[sel], 0] = rin[f, h, cols[sel]]
                    link.m_sent[h] = np.maximum(old, new)
                sender.inputs.copy_(torch.from_numpy(m_sender[..., 0]))
                link.sent.copy_(torch.from_numpy(link.m_sent))
                _, r = send_and_receive(link, sender, m_sender, ring, m_ring, m_upto, drops[t], f"tick {t}")
                resent += r
                rows.append(ring.upto.clone())
                uptos[t] = m_upto
            for h in remotes:
                for j in range(int((m_upto[h] - fed[h]).max())):
                    sel = fed[h] + 1 + j <= m_upto[h]
                    f = (fed[h] + 1 + j)[sel]
                    twin_ring[f & M, h, cols[sel]] = rin[f, h, cols[sel]]
                fed[h] = np.maximum(fed[h], m_upto[h])
            sess.run_ticks(di[t0:t1], torch.stack(rows), ring.inputs)
            twin.run_ticks(di[t0:t1], dev(uptos[t0:t1]), dev(twin_ring))
            for t in range(t0, t1):
                cls.tick(t, ALL, inputs, uptos, rin)
            compare_all(sess, cls, f"ticks {t0}..{t1 - 1}")
            equal_everything(sess, twin, False, f"ticks {t0}..{t1 - 1}")
        assert (sess.frames()[0] > 2 * R).all() and resent > SL and sess.counters()[2] == 0 and (cls.lf >= 0).any()
        for b in (sess, twin, cls):
            b.close()


# ---------------------------------------------------------------------------
# GPU 6: spectators
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_ring_host_sends_its_confirmed_inputs_to_ring_spectators_as_packets(gpu_available):
    """A ring-mode host's export_confirmed_inputs -> send_packets for all handles -> receive_packets
    into the spectators' ring -> the spectators equal the truth run, across frames 128 and 256.  The
    spectators' watermark is the minimum over the handles of what arrived; acks come back one call
    late and a tenth of the packets is lost."""
    import torch

    import test_spectator as TS
    from test_delivery_ring import Feeder
    from test_p2p_pacing import dev
    game, P, mask, chunk, ticks = G.Game.EX_GAME, 2, 0b01, 5, LOOP_T
    inputs, upto, rin = TS.host_network(game, P, mask, SL, ticks + 8)
    host = TS.start_host(game, P, mask, SL)
    spec = TS.start_spectators(game, P, SL, catchup=2)
    host.set_delivery_ring(R)
    spec.set_delivery_ring(R)
    di, du = dev(inputs, upto)
    fd = Feeder(P, mask, SL)
    feed = TS.Feed(host, R)
    out_ring, in_ring = G.DeliveryRing(R, P, SL), G.DeliveryRing(R, P, SL)
    out_ring.inputs = feed.inputs  # the host's export is the sender's ring
    seen = TS.host_truth(game, P, mask, inputs, rin, ticks + 8)
    all_handles = (1 << P) - 1
    pk = torch.zeros((P, SL, LOOP_STRIDE), dtype=torch.uint8, device="cuda")
    ln, st = (torch.zeros((P, SL), dtype=torch.int32, device="cuda") for _ in range(2))
    acked = torch.full((P, SL), G.NULL_FRAME, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(61)
    for t0 in range(0, ticks, chunk):
        t1 = min(t0 + chunk, ticks)
        fd.feed(upto[t0:t1], rin)
        host.run_ticks(di[t0:t1], du[t0:t1], fd.device())
        host.export_confirmed_inputs(feed.inputs, feed.upto, feed.last, feed.disc)
        spec.receive_host_status(feed.last.clone(), feed.disc.clone())
        newest = feed.upto[None].expand(P, SL).contiguous()
        out_ring.send_packets(all_handles, newest, acked, 0, pk, ln, st)
        assert int((ln < 0).sum()) == 0
        ln[dev(rng.random((P, SL)) < 0.1)] = 0
        acked = in_ring.upto.clone()  # the ack of the previous call's packets
        status = in_ring.receive_packets(all_handles, pk, ln, st, TS.W_)
        assert int((status < 0).sum()) == 0
        target = in_ring.upto.min(dim=0).values
        spec.run_ticks(target[None].expand(t1 - t0, SL).contiguous(), in_ring.inputs)
        TS.assert_state_is_truth(spec, seen, f"tick {t1 - 1}")
        got, sent_, to = in_ring.inputs.cpu().numpy(), feed.inputs.cpu().numpy(), in_ring.upto.cpu().numpy()
        for h in range(P):
            for s in range(SL):  # what arrived is what the host exported, frame by frame
                f = np.arange(max(0, to[h, s] - 30), to[h, s] + 1)
                np.testing.assert_array_equal(got[f & M, h, s], sent_[f & M, h, s], err_msg=f"tick {t1 - 1}, ({h}, {s})")
    cur, _ = spec.frames()
    assert cur.min() > 2 * R and spec.totals()[2] == 0 and (host.export_status()[0] == L.RB_P2P_EXPORT_OK).all()
    for b in (host, spec):
        b.close()
