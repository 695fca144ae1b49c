"""The packet codec for endpoints that carry several handles in one stream (include/ggrs_amd.h
rb_decode_input_packets_grouped, rb_encode_input_packets_grouped; ggrs_amd.EndpointGroups;
DeliveryRing.receive_packets / send_packets with groups): a remote peer with
more than one local player, and every spectator endpoint.

Every expectation comes from a model of on_input / send_pending_output for a group
(``model_decode`` / ``model_encode``) built on test_wire.on_input_reference with
ib = k * input_bytes and on oracle.wire_encode / wire_decode over the concatenated frames; every
comparison is an equality.  The seeded schedules (``decode_case`` / ``encode_case``) give every
endpoint one of a fixed list of situations; a CPU witness counts, on the model alone, that every
situation the kernels can get wrong is in them.  The same schedules drive the step header on the
host (tests/check_wire_group.cpp), plain and under the address and undefined-behaviour sanitizers.

S = 70 (one full wave and a ragged one), R = 128, a linear tensor of 160 frames, W = 8, packet
rows of 32 and 544 bytes.
"""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine library is loaded: the process then holds one HIP runtime, torch's)

import ggrs_amd as G
from ggrs_amd import _lib as L
from oracle import oracle as O
from test_wire import on_input_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "ggrs_amd", "csrc")
_TESTS = os.path.join(ROOT, "tests")
R, LIN, W, S = 128, 160, 8, 70
M = R - 1
ROOMY, TIGHT = 544, 32
SENT = -77  # what rows and entries nobody may write are prefilled with
FIRST_FRAME = 2

GROUP_SETS = {  # name: (P, groups)
    "p2-01": (2, [[0, 1]]),
    "p2-spectator": (2, None),  # EndpointGroups.spectator: both handles remote, none local
    "p3-12": (3, [[1, 2]]),
    "p4-01-23": (4, [[0, 1], [2, 3]]),
    "p4-02-13": (4, [[0, 2], [1, 3]]),
    "p4-123": (4, [[1, 2, 3]]),
    "p4-0123": (4, [[0, 1, 2, 3]]),
    "p4-3-01": (4, [[3], [0, 1]]),
}
SHAPES = [(name, ib, ring) for name in GROUP_SETS for ib in (1, 2, 4) for ring in (True, False)]
SHAPE_IDS = [f"{name}-ib{ib}-{'ring' if ring else 'linear'}" for name, ib, ring in SHAPES]


def groups_of(name):
    P, gs = GROUP_SETS[name]
    return P, (G.EndpointGroups.spectator(P) if gs is None else G.EndpointGroups(gs, P))


def seed_of(name, ib, ring):
    return 100 * list(GROUP_SETS).index(name) + 10 * ib + int(ring)


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def model_decode(raw, upto, status, eg, pk, ln, st, ring):
    """on_input for the endpoint of every group.  raw uint8 [F, P, S, ib], upto and status int32
    [P, S], pk uint8 [P, S, stride], ln / st int32 [P, S]: updated in place.  Returns
    {(lead, s): (reason, first new frame, last new frame, frames the packet carried)}."""
    F, P, n, ib = raw.shape
    stride = pk.shape[2]
    told = {}
    for lead in eg.leads:
        mem = list(eg.members(lead))
        fb = ib * len(mem)
        for s in range(n):
            last, start, k = int(upto[lead, s]), int(st[lead, s]), int(ln[lead, s])
            # the checks in the kernels' order: nothing / overlong / gap / stale / negative / linear range
            if k <= 0:
                status[lead, s], told[lead, s] = 1, ("nothing",)
                continue
            if k > stride:
                status[lead, s], told[lead, s] = -1, ("overlong",)
                continue
            if last != -1 and last + 1 < start:
                status[lead, s], told[lead, s] = -2, ("gap",)
                continue
            if last != -1 and start - 1 < last - 2 * W:
                status[lead, s], told[lead, s] = 1, ("stale",)
                continue
            if last != -1 and start - 1 < -1:
                status[lead, s], told[lead, s] = 1, ("negative",)
                continue
            if not ring and start - 1 >= F:
                status[lead, s], told[lead, s] = -1, ("range",)
                continue
            rslot = (start - 1) & (F - 1) if ring else min(max(start - 1, 0), F - 1)
            refin = raw[rslot, mem, s].tobytes()  # the members' inputs one after the other
            data = pk[lead, s, :k].tobytes()
            out, _, code = on_input_reference(last, start, data, refin, W, fb)
            if code == -1:
                whole = O.wire_decode(bytes(1), data, cap=1 << 20)  # the stream as single bytes
                status[lead, s] = -1
                told[lead, s] = ("partial", len(whole)) if whole is not None else ("malformed",)
                continue
            keep = {}
            if out:  # ring: the first R frames above `last`, no slot twice; linear: below F
                lo = min(out)
                keep = {f: b for f, b in out.items() if (f < lo + F if ring else f < F)}
            for f, b in keep.items():
                raw[f & (F - 1) if ring else f, mem, s] = np.frombuffer(b, np.uint8).reshape(len(mem), ib)
            newest = max(keep) if keep else last
            upto[mem, s] = newest  # every member's row
            status[lead, s] = 0 if keep else 1
            told[lead, s] = ("taken", min(keep), newest, len(out)) if keep else ("old",)
    return told


def model_encode(raw, eg, acked, newest, first_frame, stride, ring):
    """send_pending_output for the endpoint of every group: ({(lead, s): packet bytes}, lengths,
    start_frames); every row but the leads' keeps SENT."""
    F, P, n, ib = raw.shape
    ln = np.full((P, n), SENT, np.int32)
    st = np.full((P, n), SENT, np.int32)
    packets = {}
    for lead in eg.leads:
        mem = list(eg.members(lead))
        for s in range(n):
            a, nw = int(acked[lead, s]), int(newest[lead, s])
            start = first_frame if a == -1 else a + 1
            st[lead, s] = start
            if nw < start or start < 0 or (not ring and nw >= F):
                ln[lead, s] = 0
                continue
            if ring and nw - (start if a == -1 else a) + 1 > F:
                ln[lead, s] = -2
                continue
            slot = (lambda f: f & (F - 1)) if ring else (lambda f: f)
            ref = bytes(ib * len(mem)) if a == -1 else raw[slot(a), mem, s].tobytes()
            frames = raw[[slot(f) for f in range(start, nw + 1)]][:, mem, s].reshape(nw - start + 1, -1)
            want = O.wire_encode(ref, frames)
            ln[lead, s] = len(want) if len(want) <= stride else -1
            if len(want) <= stride:
                packets[lead, s] = want
    return packets, ln, st


# ---------------------------------------------------------------------------
# the schedules
# ---------------------------------------------------------------------------
def noise(rng, count):
    """count stream bytes in 1 .. 254: none that a run can take."""
    return rng.integers(1, 255, count, dtype=np.uint8)


def rle(stream):
    """The packet of an XOR stream (the oracle's encoder against a blank one-byte reference)."""
    return O.wire_encode(bytes(1), np.asarray(stream, np.uint8).reshape(-1, 1))


def varint(v):
    out = []
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    return bytes(out + [v])


def segments(data):
    """A well-formed packet's segments: [(is_run, length)]."""
    out, p = [], 0
    while p < len(data):
        v, sh = 0, 0
        while True:
            b = data[p]
            p += 1
            v |= (b & 0x7F) << sh
            sh += 7
            if not b & 0x80:
                break
        out.append((bool(v & 1), v >> 2 if v & 1 else v >> 1))
        if not v & 1:
            p += v >> 1
    assert p == len(data)
    return out


def run_ends_inside_a_frame(data, fb):
    at = 0
    for is_run, n in segments(data):
        at += n
        if is_run and at % fb:
            return True
    return False


def split_frame(rng, ib, k):
    """A frame's XOR bytes: zeros through member 0 and all but the last byte of member 1 (a run that
    began in the frames before ends inside member 1's input, or, 1-byte inputs, at its start), then
    changed bytes to the frame's end."""
    fb = ib * k
    return np.concatenate([np.zeros(2 * ib - 1, np.uint8), noise(rng, fb - 2 * ib + 1)])


def stream_for_length(rng, length, fb):
    """An XOR stream of whole frames whose packet has exactly `length` bytes, length 1 or >= 7:
    one run, or literal | run of zeros | literal."""
    if length == 1:
        return np.zeros(fb * -(-4 // fb), np.uint8)
    a = (length - 3) // 2
    b = length - 3 - a
    assert 1 <= a < 64 and 1 <= b < 64
    run = 4
    while (a + run + b) % fb:
        run += 1
    stream = np.concatenate([noise(rng, a), np.zeros(run, np.uint8), noise(rng, b)])
    assert len(rle(stream)) == length, (length, fb)
    return stream


DECODE_KINDS = ["new", "wrap", "ref_top", "first0", "firstN", "first_neg", "stale", "edge_stale", "gap", "malformed",
                "overlong", "cap", "cap_first", "neg_ref", "run1", "lit1", "len16", "len17", "len32", "len33", "len70",
                "bigrun", "partial", "split", "none", "range", "new"]


@functools.lru_cache(maxsize=None)
def decode_case(name, ib, ring, stride=ROOMY):
    """A receiver's tensor, watermarks and one packet per endpoint: (raw [F, P, S, ib], upto [P, S],
    pk [P, S, stride], ln, st [P, S], kinds {(lead, s): name}).  The tensor starts out full of an
    older match's bytes; rows that are no lead's hold noise nobody may read."""
    P, eg = groups_of(name)
    rng = np.random.default_rng(1000 + seed_of(name, ib, ring))
    F = R if ring else LIN
    raw = rng.integers(0, 256, (F, P, S, ib), dtype=np.uint8)
    upto = np.full((P, S), SENT, np.int32)
    pk = rng.integers(0, 256, (P, S, stride), dtype=np.uint8)  # bytes past a packet's length are noise
    ln = rng.integers(1, 30, (P, S)).astype(np.int32)          # (the leads' rows are set below)
    st = rng.integers(0, 50, (P, S)).astype(np.int32)
    kinds = {}
    for gi, lead in enumerate(eg.leads):
        mem = list(eg.members(lead))
        k = len(mem)
        fb = k * ib
        for s in range(S):
            kind = DECODE_KINDS[(s + 11 * gi) % len(DECODE_KINDS)]
            if kind in ("wrap", "ref_top", "cap", "cap_first") and not ring:
                kind = "lin_end"    # the packet runs past the tensor's last frame
            if kind == "range" and ring:
                kind = "new"
            if kind == "partial" and k == 1 and ib == 1:
                kind = "malformed"  # every stream is whole frames of one byte
            kinds[lead, s] = kind
            last = int(rng.integers(200, 1 << 30) - 8) if ring else int(rng.integers(2 * W + 8, LIN - 40))
            redo = int(rng.integers(0, 3))
            frames = None     # the packet's frames [count, fb], XORed with the reference below
            stream = None     # or the XOR stream itself
            rand = lambda count: rng.integers(0, 256, (count, fb), dtype=np.uint8)
            if kind == "new":
                frames = rand(int(rng.integers(1, 6)) + redo)
            elif kind == "wrap":
                last = int(rng.integers(2, 1 << 22)) * R + R - 3
                frames = rand(6 + redo)
            elif kind == "ref_top":
                last, redo = int(rng.integers(2, 1 << 22)) * R - 1, 0
                frames = rand(int(rng.integers(1, 5)))
            elif kind in ("first0", "firstN", "first_neg", "cap_first"):
                last, redo = -1, 0
            elif kind == "neg_ref":
                last, redo = int(rng.integers(0, 5)), 0
            elif kind == "lin_end":
                last = LIN - 4 + int(rng.integers(0, 3))
            start = last + 1 - redo
            if kind == "first0":
                start, frames = 0, rand(int(rng.integers(1, 6)))
            elif kind == "firstN":  # a first packet after the sender's delay: slot start - 1 holds an old match's bytes
                start, frames = int(rng.integers(1, 4)), rand(int(rng.integers(1, 6)))
            elif kind == "first_neg":
                start, frames = -3, rand(6)
            elif kind == "cap_first":
                start, stream = 2, np.zeros((R + 10) * fb, np.uint8)
            elif kind == "neg_ref":
                start, frames = -3, rand(12)
            elif kind == "stale":       # the reference is older than recv_inputs keeps; frames past `last` follow
                start, frames = last - 2 * W - int(rng.integers(1, 6)), rand(2 * W + 12)
            elif kind == "edge_stale":  # exactly as old as recv_inputs still keeps
                start, frames = last - 2 * W + 1, rand(2 * W + 3)
            elif kind == "gap":
                start, frames = last + 2, rand(3)
            elif kind == "cap":         # more than R new frames: a run, then two literal frames
                stream = np.concatenate([np.zeros((R + 40 + redo) * fb, np.uint8), noise(rng, 2 * fb)])
            elif kind == "lin_end":
                frames = rand(8 + redo)
            elif kind == "range":       # the reference lies at / past the tensor's end
                start = LIN + 1 + int(rng.integers(0, 3))
                last, frames = start - 1 + int(rng.integers(0, 2)), rand(2)
            elif kind == "run1":        # one run: every member holds its reference input
                unit = fb * -(-4 // fb)
                stream = np.zeros(unit * int(rng.integers(1, 31 // unit + 1)), np.uint8)
            elif kind == "lit1":        # one literal within the 32-byte head
                stream = noise(rng, fb * int(rng.integers(1, 31 // fb + 1)))
            elif kind.startswith("len"):
                stream = stream_for_length(rng, int(kind[3:]), fb)
            elif kind == "bigrun":      # a run of more than 65,536 bytes after a valid literal frame
                stream = None
            elif kind == "partial":     # whole inputs, but not whole frames of the group
                count = k * int(rng.integers(1, 4)) + int(rng.integers(1, k)) if k > 1 else 0
                stream = noise(rng, count * ib) if k > 1 else noise(rng, ib + int(rng.integers(1, ib)))
            elif kind == "split":       # held frames, then two in which the members differ in which bytes changed
                one = split_frame(rng, ib, k) if k > 1 else noise(rng, fb)
                stream = np.concatenate([np.zeros(fb * -(-4 // fb), np.uint8), one, one])
            elif kind in ("malformed", "overlong", "none"):
                frames = rand(3 + redo)
            blank = last == -1 or start - 1 == -1
            ref = np.zeros(fb, np.uint8) if blank else rng.integers(0, 256, fb, dtype=np.uint8)
            if not blank and (ring or 0 <= start - 1 < F):
                raw[(start - 1) & M if ring else start - 1, mem, s] = ref.reshape(k, ib)
            if kind == "bigrun":
                big = -(-65537 // fb) * fb  # whole frames, more than 65,536 bytes
                data = rle(noise(rng, fb)) + varint((big << 2) | 1) + rle(noise(rng, fb))
            else:
                if stream is None:
                    stream = (frames ^ ref[None, :]).reshape(-1)
                data = rle(stream)
            if kind == "malformed":  # a valid first segment, then a header that runs off the packet's end
                data += bytes([0x80]) if s % 2 else bytes([0x0A, 1, 2])
            assert len(data) <= stride, (kind, len(data))
            pk[lead, s, :len(data)] = np.frombuffer(data, np.uint8)
            upto[mem, s] = last
            if s % 5 == 0 and k > 1:  # only the lead's watermark is read
                upto[mem[1:], s] = last - 3
            st[lead, s] = start
            ln[lead, s] = {"overlong": stride + 1 + int(rng.integers(0, 1 << 20)), "none": -5 * (s % 2)}.get(kind, len(data))
    for a in (raw, upto, pk, ln, st):
        a.setflags(write=False)
    return raw, upto, pk, ln, st, kinds


ENCODE_KINDS = ["new", "nothing", "first", "first_none", "fit_R", "over_R", "over_R5", "first_fit", "first_over", "exact",
                "over", "split", "held", "lin_past", "long"]


@functools.lru_cache(maxsize=None)
def encode_case(name, ib, ring):
    """A sender's tensor and one (acked, newest) per endpoint: (raw [F, P, S, ib], acked, newest
    [P, S], kinds).  Rows that are no lead's hold noise nobody may read."""
    P, eg = groups_of(name)
    rng = np.random.default_rng(2000 + seed_of(name, ib, ring))
    F = R if ring else LIN
    slot = (lambda f: f & M) if ring else (lambda f: f)
    raw = rng.integers(0, 256, (F, P, S, ib), dtype=np.uint8)
    for h in range(P):  # every third column in blocks of held inputs: runs
        for s in range(h % 3, S, 3):
            raw[:, h, s] = np.repeat(rng.integers(0, 256, (F // 8, ib), dtype=np.uint8), 8, axis=0)
    acked = rng.integers(0, 100, (P, S)).astype(np.int32)
    newest = (acked + rng.integers(0, 9, (P, S))).astype(np.int32)
    kinds = {}
    for gi, lead in enumerate(eg.leads):
        mem = list(eg.members(lead))
        k = len(mem)
        fb = k * ib
        for s in range(S):
            kind = ENCODE_KINDS[(s + 7 * gi) % len(ENCODE_KINDS)]
            if not ring and kind in ("fit_R", "over_R", "over_R5", "first_fit", "first_over"):
                kind = "new"
            if ring and kind == "lin_past":
                kind = "new"
            kinds[lead, s] = kind
            a = int(rng.integers(0, 1 << 30) - R - 8) if ring else int(rng.integers(0, LIN - 60))
            if kind in ("new", "held", "long"):
                nw = a + int(rng.integers(1, 6))
                if kind == "held":
                    raw[:, mem, s] = raw[0, mem, s]
                    nw = a + int(rng.integers(4, 40))
                if kind == "long":  # nothing to compress: the packet outgrows the 32-byte window
                    raw[:, mem, s] = rng.integers(0, 256, (F, k, ib), dtype=np.uint8)
                    nw = a + 2 + 64 // fb
            elif kind == "nothing":
                nw = a - int(rng.integers(0, 4))
            elif kind == "first":
                a, nw = -1, FIRST_FRAME + int(rng.integers(0, 5))
            elif kind == "first_none":
                a, nw = -1, FIRST_FRAME - 1 - int(rng.integers(0, 3))
            elif kind == "fit_R":       # (held inputs: R frames of up to 16 bytes fit a row only as runs)
                nw = a + R - 1
                raw[:, mem, s] = raw[0, mem, s]
            elif kind == "over_R":
                nw = a + R
            elif kind == "over_R5":
                nw = a + R + 5
            elif kind == "first_fit":
                a, nw = -1, FIRST_FRAME + R - 1
                raw[:, mem, s] = 0
            elif kind == "first_over":
                a, nw = -1, FIRST_FRAME + R
            elif kind == "lin_past":
                nw = LIN + int(rng.integers(0, 3))
            else:  # the XOR stream is given: a packet of exactly TIGHT bytes, one a little longer, a run ending inside a member
                if kind == "split":
                    one = split_frame(rng, ib, k) if k > 1 else noise(rng, fb)
                    stream = np.concatenate([np.zeros(fb * -(-4 // fb), np.uint8), one, one, np.zeros(fb * -(-4 // fb), np.uint8)])
                else:
                    stream = stream_for_length(rng, TIGHT if kind == "exact" else TIGHT + 1 + int(rng.integers(0, 4)), fb)
                x = stream.reshape(-1, k, ib)
                f = np.arange(a + 1, a + 1 + len(x))
                raw[slot(f)[:, None], np.array(mem)[None, :], s] = x ^ raw[slot(a), mem, s][None]
                nw = a + len(x)
            acked[lead, s], newest[lead, s] = a, nw
    for x in (raw, acked, newest):
        x.setflags(write=False)
    return raw, acked, newest, kinds


@functools.lru_cache(maxsize=None)
def decoded(name, ib, ring):
    """The model's answer to decode_case: (raw, upto, status, told)."""
    P, eg = groups_of(name)
    raw0, upto0, pk, ln, st, _ = decode_case(name, ib, ring)
    raw, upto, status = raw0.copy(), upto0.copy(), np.full((P, S), SENT, np.int32)
    told = model_decode(raw, upto, status, eg, pk, ln, st, ring)
    return raw, upto, status, told


@functools.lru_cache(maxsize=None)
def encoded(name, ib, ring, stride):
    P, eg = groups_of(name)
    raw, acked, newest, _ = encode_case(name, ib, ring)
    return model_encode(raw, eg, acked, newest, FIRST_FRAME, stride, ring)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_declarations_and_exports():
    header = open(os.path.join(ROOT, "include", "ggrs_amd.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("rb_decode_input_packets_grouped", "rb_encode_input_packets_grouped"):
        assert re.search(r"^rb_status " + name + r"\(int32_t device, void\* stream, uint32_t group_masks, int32_t num_players,",
                         header, re.M), name
        assert f"| `{name}` |" in integration
    lib = L.load()
    sig = {name: (res, args) for name, res, args in L.SIGNATURES}
    P_, I_, U_, Q_ = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64
    want = {"rb_decode_input_packets_grouped": [I_, P_, U_, I_, I_, I_, I_, P_, Q_, P_, P_, P_, I_, I_, P_, P_],
            "rb_encode_input_packets_grouped": [I_, P_, U_, I_, I_, I_, P_, I_, I_, I_, P_, P_, P_, Q_, P_, P_]}
    for name, args in want.items():
        assert sig[name] == (I_, args)
        fn = getattr(lib, name)
        assert fn.restype is I_ and fn.argtypes == args
    from ggrs_amd.endpoint_groups import EndpointGroups
    from ggrs_amd.wire import decode_packets_grouped, encode_packets_grouped
    assert G.EndpointGroups is EndpointGroups
    assert G.decode_packets_grouped is decode_packets_grouped and G.encode_packets_grouped is encode_packets_grouped
    import inspect
    for fn in (G.DeliveryRing.receive_packets, G.DeliveryRing.send_packets):
        assert inspect.signature(fn).parameters["groups"].default is None


def test_endpoint_groups_object():
    eg = G.EndpointGroups([[3], [1, 0]], 4)
    assert eg.packed == 0b1000 | (0b0011 << 8) and eg.lead_mask == 0b1001
    assert eg.members(0) == (0, 1) and eg.members(3) == (3,)
    assert G.EndpointGroups([0b1000, 0b0011], 4).packed == eg.packed
    sp = G.EndpointGroups.spectator(3)
    assert sp.packed == 0b111 and sp.lead_mask == 1 and sp.members(0) == (0, 1, 2)
    t = np.arange(2 * 4 * 3).reshape(2, 4, 3)
    out = eg.spread(t.copy())
    np.testing.assert_array_equal(out[:, 1], t[:, 0])
    np.testing.assert_array_equal(out[:, [0, 2, 3]], t[:, [0, 2, 3]])
    tt = torch.from_numpy(t.copy())
    assert eg.spread(tt) is tt and np.array_equal(tt.numpy(), out)
    for bad in ([[0, 0]], [[0], [0, 1]], [[4]], [[]], [], [0], [[0], [1], [2], [3], [0]]):
        with pytest.raises(ValueError):
            G.EndpointGroups(bad, 4)
    with pytest.raises(KeyError):
        eg.members(1)


@functools.lru_cache(maxsize=None)
def check_program(sanitized=False):
    import tempfile
    exe = os.path.join(tempfile.mkdtemp(prefix="check_wire_group_"), "check_wire_group")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O1"]
    subprocess.run(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-I", _CSRC, "-o", exe,
                    os.path.join(_TESTS, "check_wire_group.cpp")], check=True)
    return exe


def hexof(b):
    return bytes(b).hex() if len(b) else "-"


def run_check(exe, mode, lines, tmp_path):
    path = tmp_path / f"{mode}.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, mode, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-1000:] + r.stderr[-4000:]
    return r.stdout.splitlines()


def host_decode(exe, tmp_path, ib, k, ring, F, stride, rows):
    """rows: (last, start, n, packet bytes held, column uint8 [F, k, ib]) -> (status, decoded, newest, column)."""
    lines = [f"{ib} {k} {int(ring)} {F} {W} {stride} {len(rows)}"]
    lines += [f"{last} {start} {n} {hexof(data)} {hexof(col.tobytes())}" for last, start, n, data, col in rows]
    out = []
    for line in run_check(exe, "decode", lines, tmp_path):
        code, dec, newest, col = line.split()
        out.append((int(code), int(dec), int(newest), np.frombuffer(bytes.fromhex(col), np.uint8).reshape(F, k, ib)))
    assert len(out) == len(rows)
    return out


def host_encode(exe, tmp_path, ib, k, ring, F, stride, first_frame, rows):
    """rows: (acked, newest, column) -> (length, start, packet bytes)."""
    lines = [f"{ib} {k} {int(ring)} {F} {first_frame} {stride} {len(rows)}"]
    lines += [f"{a} {nw} {hexof(col.tobytes())}" for a, nw, col in rows]
    out = []
    for line in run_check(exe, "encode", lines, tmp_path):
        n, start, data = line.split()
        out.append((int(n), int(start), b"" if data == "-" else bytes.fromhex(data)))
    assert len(out) == len(rows)
    return out


def test_known_answers_of_the_oracle_and_of_the_step_header(tmp_path):
    exe = check_program()
    # P = 2, 1-byte inputs, group {0, 1}, no ack, one frame (0x01, 0x02): one literal of two bytes
    assert O.wire_encode(bytes(2), np.array([[1, 2]], np.uint8)) == bytes([0x04, 0x01, 0x02])
    col = np.zeros((R, 2, 1), np.uint8)
    col[0, :, 0] = (1, 2)
    assert host_encode(exe, tmp_path, 1, 2, True, R, 32, 0, [(-1, 0, col)]) == [(3, 0, bytes([0x04, 0x01, 0x02]))]
    (code, dec, newest, got), = host_decode(exe, tmp_path, 1, 2, True, R, 32, [(-1, 0, 3, bytes([4, 1, 2]), np.zeros_like(col))])
    assert (code, dec, newest) == (0, 1, 0) and (got == col).all()
    # a 16-byte frame equal to its reference: one run of 16 zero bytes, header 16 << 2 | 1
    ref = np.arange(16, dtype=np.uint8) + 1
    assert O.wire_encode(ref.tobytes(), ref[None, :]) == bytes([0x41])
    col = np.zeros((R, 4, 4), np.uint8)
    col[4] = col[5] = ref.reshape(4, 4)
    assert host_encode(exe, tmp_path, 4, 4, True, R, 32, 0, [(4, 5, col)]) == [(1, 5, bytes([0x41]))]
    col[5] = 0
    (code, dec, newest, got), = host_decode(exe, tmp_path, 4, 4, True, R, 32, [(4, 5, 1, bytes([0x41]), col)])
    assert (code, dec, newest) == (0, 1, 5) and (got[5] == ref.reshape(4, 4)).all()
    # one member's input more than whole frames: whole inputs, not whole frames
    (code, dec, newest, got), = host_decode(exe, tmp_path, 1, 2, True, R, 32, [(-1, 0, 4, bytes([6, 1, 2, 3]), np.zeros((R, 2, 1), np.uint8))])
    assert (code, dec, newest) == (-1, 0, -1) and not got.any()


def host_schedules(exe, tmp_path, name, ib, ring):
    """decode_case and encode_case of one shape through the step header on the host, against the model."""
    P, eg = groups_of(name)
    F = R if ring else LIN
    raw0, upto0, pk, ln, st, _ = decode_case(name, ib, ring)
    want_raw, want_upto, want_status, told = decoded(name, ib, ring)
    for lead in eg.leads:
        mem = list(eg.members(lead))
        rows = [(int(upto0[lead, s]), int(st[lead, s]), int(ln[lead, s]), pk[lead, s, :min(max(int(ln[lead, s]), 0), ROOMY)],
                 raw0[:, mem, s]) for s in range(S)]
        for s, (code, dec, newest, col) in enumerate(host_decode(exe, tmp_path, ib, len(mem), ring, F, ROOMY, rows)):
            what = f"{name} ib {ib} ring {ring}: decode ({lead}, {s})"
            assert code == want_status[lead, s], what
            assert dec == int(told[lead, s][0] in ("taken", "old")), what
            assert newest == (want_upto[lead, s] if dec else upto0[lead, s]), what
            np.testing.assert_array_equal(col, want_raw[:, mem, s], err_msg=what)
    raw, acked, newest, _ = encode_case(name, ib, ring)
    for stride in (ROOMY, TIGHT):
        packets, wln, wst = encoded(name, ib, ring, stride)
        for lead in eg.leads:
            mem = list(eg.members(lead))
            rows = [(int(acked[lead, s]), int(newest[lead, s]), raw[:, mem, s]) for s in range(S)]
            for s, (n, start, data) in enumerate(host_encode(exe, tmp_path, ib, len(mem), ring, F, stride, FIRST_FRAME, rows)):
                what = f"{name} ib {ib} ring {ring} stride {stride}: encode ({lead}, {s})"
                assert (n, start) == (wln[lead, s], wst[lead, s]), what
                assert data == packets.get((lead, s), b""), what


@pytest.mark.parametrize("name,ib,ring", SHAPES, ids=SHAPE_IDS)
def test_the_step_header_on_the_host_equals_the_model(tmp_path, name, ib, ring):
    host_schedules(check_program(), tmp_path, name, ib, ring)


def test_the_step_header_under_the_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined, every packet in a heap
    buffer of exactly its bytes and every column in one of exactly its frames: the schedules, then
    rows of random bytes, lengths, start frames and watermarks through every instantiation."""
    exe = check_program(sanitized=True)
    for name, ib, ring in SHAPES:
        host_schedules(exe, tmp_path, name, ib, ring)
    for seed in (1, 2):
        r = subprocess.run([exe, "fuzz", str(seed), "3000"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("fuzz ok") and not r.stderr, r.stdout[-500:] + r.stderr[-4000:]


def test_schedules_hold_every_case_the_kernels_can_get_wrong():
    """On the model alone: the counts of every situation, over the schedules the host and GPU tests run."""
    seen = dict.fromkeys(("nothing", "overlong", "gap", "stale", "negative", "range", "malformed", "partial",
                          "partial_whole_inputs", "bigrun", "first_no_earlier_frame", "first_after_old_frames", "split",
                          "len1", "len16", "len17", "len32", "len33", "len_over_64", "cap", "wrap", "ref_top", "resent",
                          "group_of_one", "sixteen_byte_frames", "member_rows_differ", "linear_end"), 0)
    for name, ib, ring in SHAPES:
        P, eg = groups_of(name)
        raw0, upto0, pk, ln, st, kinds = decode_case(name, ib, ring)
        raw, upto, status, told = decoded(name, ib, ring)
        leads = list(eg.leads)
        for (lead, s), kind in kinds.items():
            mem = list(eg.members(lead))
            fb = ib * len(mem)
            why = told[lead, s]
            last, start, n = int(upto0[lead, s]), int(st[lead, s]), int(ln[lead, s])
            if why[0] in seen and why[0] not in ("malformed", "partial"):
                seen[why[0]] += 1
            if why[0] == "partial":
                seen["partial"] += 1
                seen["partial_whole_inputs"] += len(mem) > 1 and why[1] % ib == 0 and why[1] % fb != 0
            if why[0] == "malformed" and kind == "bigrun":
                segs = segments(pk[lead, s, :n].tobytes())
                assert max(x for r, x in segs if r) > 65536 and sum(x for _, x in segs) % fb == 0
                seen["bigrun"] += 1
            elif why[0] == "malformed":
                seen["malformed"] += 1
            if why[0] == "taken":
                _, lo, hi, carried = why
                assert status[lead, s] == 0 and (upto[mem, s] == hi).all()
                seen["first_no_earlier_frame"] += last == -1 and start == 0
                seen["first_after_old_frames"] += last == -1 and start > 0 and bool(raw0[(start - 1) % len(raw0), mem, s].any())
                seen["split"] += len(mem) > 1 and run_ends_inside_a_frame(pk[lead, s, :n].tobytes(), fb)
                seen["len_over_64"] += n > 64
                for size in (1, 16, 17, 32, 33):
                    seen[f"len{size}"] += n == size
                seen["cap"] += ring and carried > R and hi - lo + 1 == R
                seen["wrap"] += ring and hi & M < lo & M
                seen["ref_top"] += ring and last != -1 and (start - 1) & M == M
                seen["resent"] += start <= last
                seen["group_of_one"] += len(mem) == 1
                seen["sixteen_byte_frames"] += fb == 16
                seen["member_rows_differ"] += len(mem) > 1 and bool((upto0[mem[1:], s] != last).any())
                seen["linear_end"] += (not ring) and hi == LIN - 1 and carried > hi - lo + 1
        for h in range(P):  # what is no lead's is nobody's; what is no member's is untouched
            if h not in leads:
                assert (status[h] == SENT).all()
            if not any(h in eg.members(x) for x in leads):
                assert (upto[h] == SENT).all()
                np.testing.assert_array_equal(raw[:, h], raw0[:, h])
    assert all(v >= 1 for v in seen.values()), seen
    enc = dict.fromkeys(("nothing", "too_long_at_32", "overrun", "exactly_R", "first_exactly_R", "fits_32_exactly", "first",
                         "split", "past_32", "past_64", "group_of_one", "sixteen_byte_frames", "linear_past"), 0)
    for name, ib, ring in SHAPES:
        P, eg = groups_of(name)
        raw, acked, newest, kinds = encode_case(name, ib, ring)
        roomy, tight = encoded(name, ib, ring, ROOMY), encoded(name, ib, ring, TIGHT)
        assert (roomy[1] != -1).all() and (roomy[2] == tight[2]).all()
        for (lead, s), kind in kinds.items():
            k = len(eg.members(lead))
            a, nw, n, nt = int(acked[lead, s]), int(newest[lead, s]), int(roomy[1][lead, s]), int(tight[1][lead, s])
            enc["nothing"] += n == 0
            enc["overrun"] += n == -2 and nt == -2
            enc["too_long_at_32"] += nt == -1 and TIGHT < n <= TIGHT + 5
            enc["exactly_R"] += n > 0 and a != -1 and nw - a + 1 == R
            enc["first_exactly_R"] += n > 0 and a == -1 and nw - FIRST_FRAME + 1 == R
            enc["first"] += n > 0 and a == -1
            enc["fits_32_exactly"] += n == TIGHT and nt == TIGHT
            enc["split"] += k > 1 and n > 0 and run_ends_inside_a_frame(roomy[0][lead, s], k * ib)
            enc["past_32"] += n > 32
            enc["past_64"] += n > 64
            enc["group_of_one"] += k == 1 and n > 0
            enc["sixteen_byte_frames"] += k * ib == 16 and n > 0
            enc["linear_past"] += (not ring) and nw >= LIN and n == 0
            if kind in ("over_R", "over_R5", "first_over"):
                assert n == -2
    assert all(v >= 1 for v in enc.values()), enc


# ---------------------------------------------------------------------------
# the device calls: numpy in, numpy out, every tensor between guard regions
# ---------------------------------------------------------------------------
def call_decode(raw, upto, status, packed, pk, ln, st, ring, max_prediction=W, P=None, all_mask=None, **over):
    """rb_decode_input_packets_grouped on copies of the arrays (all_mask: rb_decode_input_packets_all
    with that handle mask instead): (rb_status, raw, upto, status)."""
    import torch
    from test_wire_ring import Guarded
    lib = L.load()
    F, P_, n, ib = raw.shape
    stride = pk.shape[2]
    g = [Guarded(a) for a in (raw, upto, status, pk, ln, st)]
    graw, gupto, gstatus, gpk, gln, gst = g
    fn = lib.rb_decode_input_packets_grouped if all_mask is None else lib.rb_decode_input_packets_all
    rc = fn(0, None, packed if all_mask is None else all_mask, P_ if P is None else P, n, over.get("ib", ib), max_prediction, gpk.ptr(), stride,
            gln.ptr(), gst.ptr(), graw.ptr(), F, over.get("ring_frames", F if ring else 0), gupto.ptr(), gstatus.ptr())
    torch.cuda.synchronize()
    out = [x.read() for x in g]
    for before, after in zip((pk, ln, st), out[3:]):
        np.testing.assert_array_equal(after, before, err_msg="decode wrote one of its inputs")
    return rc, out[0], out[1], out[2]


def call_encode(raw, packed, acked, newest, first_frame, stride, ring, P=None, all_mask=None, fill=0xEE, **over):
    """rb_encode_input_packets_grouped on copies: (rb_status, pk [P, S, stride], ln, st); rows nobody
    writes keep `fill` / SENT."""
    import torch
    from test_wire_ring import Guarded
    lib = L.load()
    F, P_, n, ib = raw.shape
    g = [Guarded(a) for a in (raw, acked, newest, np.full((P_, n, stride), fill, np.uint8), np.full((P_, n), SENT, np.int32),
                              np.full((P_, n), SENT, np.int32))]
    graw, gack, gnew, gpk, gln, gst = g
    fn = lib.rb_encode_input_packets_grouped if all_mask is None else lib.rb_encode_input_packets_all
    rc = fn(0, None, packed if all_mask is None else all_mask, P_ if P is None else P, n, over.get("ib", ib), graw.ptr(), F,
            over.get("ring_frames", F if ring else 0), first_frame, gack.ptr(), gnew.ptr(), gpk.ptr(over.get("off", 0)), stride,
            gln.ptr(), gst.ptr())
    torch.cuda.synchronize()
    out = [x.read() for x in g]
    for before, after in zip((raw, acked, newest), out[:3]):
        np.testing.assert_array_equal(after, before, err_msg="encode wrote one of its inputs")
    return rc, out[3], out[4], out[5]


def assert_packets(pk, ln, st, want, what, fill=0xEE):
    """Lengths, start frames and the packets' bytes against model_encode's; rows that are no lead's,
    and an overrun endpoint's, keep their fill.  Bytes past a packet's length are unspecified."""
    packets, wln, wst = want
    np.testing.assert_array_equal(ln, wln, err_msg=f"lengths, {what}")
    np.testing.assert_array_equal(st, wst, err_msg=f"start frames, {what}")
    for h in range(pk.shape[0]):
        for s in range(pk.shape[1]):
            if wln[h, s] in (SENT, -2):
                assert (pk[h, s] == fill).all(), f"{what}: row ({h}, {s}) was written"
            elif wln[h, s] > 0:
                assert pk[h, s, :wln[h, s]].tobytes() == packets[h, s], f"{what}: packet ({h}, {s})"


# ---------------------------------------------------------------------------
# GPU 1: decode and encode against the model
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,ib,ring", SHAPES, ids=SHAPE_IDS)
def test_gpu_grouped_decode_matches_the_model(gpu_available, name, ib, ring):
    P, eg = groups_of(name)
    raw0, upto0, pk, ln, st, _ = decode_case(name, ib, ring)
    want_raw, want_upto, want_status, _ = decoded(name, ib, ring)
    rc, raw, upto, status = call_decode(raw0, upto0, np.full((P, S), SENT, np.int32), eg.packed, pk, ln, st, ring)
    assert rc == L.RB_OK
    np.testing.assert_array_equal(status, want_status, err_msg="status: the leads' rows, and SENT everywhere else")
    np.testing.assert_array_equal(upto, want_upto, err_msg="upto: every member's row, and no other")
    np.testing.assert_array_equal(raw, want_raw, err_msg="the tensor: written entries, and every entry not written")
    for lead in eg.leads:
        mem = list(eg.members(lead))
        took = np.isin(status[lead], (0,))
        assert (upto[mem][:, took] == upto[lead, took]).all()
    assert {0, 1, -1, -2, SENT} >= set(np.unique(status).tolist()) >= {0, 1, -1, -2}


@pytest.mark.gpu
@pytest.mark.parametrize("name,ib,ring", SHAPES, ids=SHAPE_IDS)
def test_gpu_grouped_encode_matches_the_oracle(gpu_available, name, ib, ring):
    P, eg = groups_of(name)
    raw, acked, newest, _ = encode_case(name, ib, ring)
    for stride in (ROOMY, TIGHT):
        rc, pk, ln, st = call_encode(raw, eg.packed, acked, newest, FIRST_FRAME, stride, ring)
        assert rc == L.RB_OK
        assert_packets(pk, ln, st, encoded(name, ib, ring, stride), f"stride {stride}")
        assert (ln == -1).any() == (stride == TIGHT) and (ln == 0).any() and ((ln == -2).any() == ring)


# ---------------------------------------------------------------------------
# GPU 2: a group of one is the _all call of that handle, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ring", [True, False], ids=["ring", "linear"])
@pytest.mark.parametrize("ib", [1, 2, 4])
def test_gpu_a_group_of_one_equals_the_all_call(gpu_available, ib, ring):
    name = "p4-3-01"
    P, eg = groups_of(name)
    one = G.EndpointGroups([[3]], P)
    raw0, upto0, pk, ln, st, _ = decode_case(name, ib, ring)
    status0 = np.full((P, S), SENT, np.int32)
    old = call_decode(raw0, upto0, status0, 0, pk, ln, st, ring, all_mask=0b1000)
    new = call_decode(raw0, upto0, status0, one.packed, pk, ln, st, ring)
    assert old[0] == new[0] == L.RB_OK
    for a, b, what in zip(old[1:], new[1:], ("inputs", "upto", "status")):
        np.testing.assert_array_equal(b, a, err_msg=what)
    assert {0, 1, -1, -2} <= set(np.unique(new[3][3]).tolist()) and (new[1] != raw0).any()
    raw, acked, newest, _ = encode_case(name, ib, ring)
    for stride in (ROOMY, TIGHT, 48):
        old = call_encode(raw, 0, acked, newest, FIRST_FRAME, stride, ring, all_mask=0b1000)
        new = call_encode(raw, one.packed, acked, newest, FIRST_FRAME, stride, ring)
        assert old[0] == new[0] == L.RB_OK
        for a, b, what in zip(old[1:], new[1:], ("packets, every byte of every row", "lengths", "start frames")):
            np.testing.assert_array_equal(b, a, err_msg=f"{what}, stride {stride}")
        assert (new[2][3] > 32).any() or stride == TIGHT


# ---------------------------------------------------------------------------
# GPU 3: validation
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_invalid_requests_touch_nothing(gpu_available):
    import torch
    name, ib = "p4-01-23", 1
    P, eg = groups_of(name)
    raw0, upto0, pk, ln, st, _ = decode_case(name, ib, True)
    status0 = np.full((P, S), SENT, np.int32)
    pack = lambda *masks: sum(m << (8 * i) for i, m in enumerate(masks))
    bad_groups = [("no group", 0), ("a bit at num_players", pack(0b10011)), ("a bit at num_players, second group", pack(0b0011, 0b10100)),
                  ("two groups share a handle", pack(0b0011, 0b0110)), ("the same group twice", pack(0b0011, 0, 0b0011)),
                  ("a bit above the handles", pack(0b0011, 0b1100, 0x80))]
    bad_decode = [(w, dict(packed=g)) for w, g in bad_groups] + [
        ("stride 40", dict(pk=np.ascontiguousarray(pk[:, :, :40]))), ("stride 16", dict(pk=np.ascontiguousarray(pk[:, :, :16]))),
        ("ring of 96", dict(raw=raw0[:96], ring_frames=96)), ("ring of 64", dict(raw=raw0[:64], ring_frames=64)),
        ("frames != ring", dict(raw=np.concatenate([raw0, raw0]), ring_frames=R)), ("2W == R", dict(max_prediction=R // 2)),
        ("W == 0", dict(max_prediction=0)), ("five players", dict(P=5)), ("no players", dict(P=0)),
        ("3-byte inputs", dict(ib=3)), ("8-byte inputs", dict(ib=8)), ("0-byte inputs", dict(ib=0))]
    for what, kw in bad_decode:
        a = dict(raw=raw0, upto=upto0, status=status0, packed=eg.packed, pk=pk, ln=ln, st=st, ring=True)
        a.update(kw)
        rc, raw, upto, status = call_decode(**a)
        assert rc == L.RB_INVALID_REQUEST, what
        np.testing.assert_array_equal(raw, a["raw"], err_msg=what)
        np.testing.assert_array_equal(upto, upto0, err_msg=what)
        np.testing.assert_array_equal(status, status0, err_msg=what)
    rc, _, _, status = call_decode(raw0, upto0, status0, eg.packed, pk, ln, st, True, max_prediction=R // 2 - 1)
    assert rc == L.RB_OK and (status[[0, 2]] != SENT).all() and (status[[1, 3]] == SENT).all()
    eraw, acked, newest, _ = encode_case(name, ib, True)
    bad_encode = [(w, dict(packed=g)) for w, g in bad_groups] + [
        ("stride 40", dict(stride=40)), ("stride 16", dict(stride=16)), ("ring of 96", dict(raw=eraw[:96], ring_frames=96)),
        ("ring of 100", dict(raw=eraw[:100], ring_frames=100)), ("frames != ring", dict(raw=np.concatenate([eraw, eraw]), ring_frames=R)),
        ("five players", dict(P=5)), ("3-byte inputs", dict(ib=3)), ("packets 8 bytes off", dict(off=8)),
        ("packets 4 bytes off", dict(off=4))]
    for what, kw in bad_encode:
        a = dict(raw=eraw, packed=eg.packed, acked=acked, newest=newest, first_frame=FIRST_FRAME, stride=ROOMY, ring=True)
        a.update(kw)
        rc, epk, eln, est = call_encode(**a)
        assert rc == L.RB_INVALID_REQUEST, what
        assert (epk == 0xEE).all() and (eln == SENT).all() and (est == SENT).all(), what
    ring = G.DeliveryRing(R, P, S)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(pk=pk, ln=ln, st=st, acked=acked, newest=newest).items()}
    with pytest.raises(ValueError):
        ring.receive_packets(0b0011, t["pk"], t["ln"], t["st"], W, groups=eg)  # neither omitted nor the lead mask
    with pytest.raises(ValueError):
        ring.send_packets(None, t["newest"], t["acked"], 0, t["pk"], t["ln"], t["st"], groups=[[0, 1], [1, 2]])
    with pytest.raises(G.InvalidRequest):
        ring.receive_packets(None, t["pk"], t["ln"], t["st"], R, groups=eg)
    assert (ring.upto == G.NULL_FRAME).all() and not ring.inputs.any()
    status = ring.receive_packets(eg.lead_mask, t["pk"], t["ln"], t["st"], W, groups=eg)
    assert (status[[0, 2]] != 0).any() or (ring.upto[[0, 2]] != G.NULL_FRAME).any()


# ---------------------------------------------------------------------------
# GPU 4: round trip
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_round_trip_between_rings_far_apart_with_late_acks(gpu_available):
    """DeliveryRing.send_packets -> receive_packets with the spectator group of P = 4, 4-byte inputs
    (16-byte frames), over 20 calls: every session counts from its own start, hundreds of frames
    apart; the sender learns the receiver's watermark one call late, so every packet but the first
    carries frames the receiver has.  After every call the receiver's slots of the frames it has
    hold the sender's inputs and its watermark is the sender's newest, on every member's row."""
    import torch
    P, calls = 4, 20
    eg = G.EndpointGroups.spectator(P)
    rng = np.random.default_rng(77)
    base = (rng.integers(1, 3000, S) * 7).astype(np.int64)  # session s counts its frames from base[s]
    base[::9] = 0
    assert np.ptp(base) > 4 * R
    per_call = rng.integers(0, 2 * W, (calls, S))  # (an ack one call late is then at most 2 W frames behind)
    total = int(per_call.sum(axis=0).max()) + 8
    truth = rng.integers(0, 1 << 32, (total, P, S), dtype=np.uint64).astype(np.uint32)  # truth[j, :, s]: frame base[s] + j
    truth[:, :, ::2] = np.repeat(truth[::8, :, ::2], 8, axis=0)[:total]  # held inputs: runs inside and across members
    send, recv = (G.DeliveryRing(R, P, S, dtype=torch.int32) for _ in range(2))
    pk = torch.zeros((P, S, ROOMY), dtype=torch.uint8, device="cuda")
    ln, st = (torch.full((P, S), SENT, dtype=torch.int32, device="cuda") for _ in range(2))
    m_send = np.zeros((R, P, S), np.uint32)
    made = np.zeros(S, np.int64)  # frames of each session produced so far
    # every match is under way: the frame before a session's first is acked and blank on both sides
    before0 = torch.from_numpy(np.broadcast_to((base - 1).astype(np.int32), (P, S)).copy()).cuda()
    acked = before0.clone()
    recv.upto.copy_(before0)
    sizes = set()
    for c in range(calls):
        for s in range(S):
            j = np.arange(made[s], made[s] + per_call[c, s])
            m_send[(base[s] + j) & M, :, s] = truth[j, :, s]
        made += per_call[c]
        send.inputs.copy_(torch.from_numpy(m_send.view(np.int32)))
        newest = torch.from_numpy(np.broadcast_to((base + made - 1).astype(np.int32), (P, S)).copy()).cuda()
        before = recv.upto.clone()
        send.send_packets(None, newest, acked, 0, pk, ln, st, groups=eg)
        acked = before  # what the receiver held before this call is what the sender knows at the next
        status = recv.receive_packets(eg.lead_mask, pk, ln, st, W, groups=eg)
        hl, hst = ln.cpu().numpy(), status.cpu().numpy()
        assert (hl[0] >= 0).all() and (hl[1:] == SENT).all() and (hst[0] >= 0).all(), f"call {c}"
        sizes |= set(hl[0].tolist())
        np.testing.assert_array_equal(recv.upto.cpu().numpy(), np.broadcast_to(base + made - 1, (P, S)), err_msg=f"upto, call {c}")
        got = recv.inputs.cpu().numpy().view(np.uint32)
        for s in range(S):
            j = np.arange(max(0, made[s] - R), made[s])
            np.testing.assert_array_equal(got[(base[s] + j) & M, :, s], truth[j, :, s], err_msg=f"call {c}, session {s}")
    assert max(sizes) > 64 and int(made.max()) > R


# ---------------------------------------------------------------------------
# GPU 5: spectators follow their host over datagrams
# ---------------------------------------------------------------------------
SPEC_CHUNK, SPEC_SEED = 5, 0x5BEC
EPOCH_MS, TICK_MS, FLIGHT_MS = 1_700_000_000_000, 16, 3
# name: game, local mask of the host, ticks, the tick player 1 is disconnected at, packet row, datagram row (31 + 5 P + the packet row)
SPEC_RUNS = {"exgame-disconnect": (G.Game.EX_GAME, 0b01, 300, 100, 128, 192),
             "stub-8-byte-frames": (G.Game.STUB, 0b10, 150, None, 544, 592)}


def spectator_losses(ticks, n=S):
    """[calls, 2, n] bool: the seeded tenth of the Input datagrams (0) and of the InputAcks (1) that never arrive."""
    return np.random.default_rng(SPEC_SEED).random((ticks // SPEC_CHUNK, 2, n)) < 0.1


@pytest.mark.parametrize("name", list(SPEC_RUNS))
def test_the_spectator_loop_never_outgrows_its_row_on_the_model(name):
    """On the model alone, with the loop's seed, row size and ack lag: the frames pending per
    packet.  The host's confirmed frame is at most DELAY ahead of its tick and at most 6 frames
    behind that (the schedule's remote lag), so frames pending <= the simulated count + 6; a frame's
    bytes and at most three header bytes must fit the packet row, and the span the ring's R."""
    import test_spectator as TS
    game, _, ticks, _, row, dg_row = SPEC_RUNS[name]
    fb = 2 * (4 if game == G.Game.STUB else 1)
    lost = spectator_losses(ticks)
    newest = np.zeros(S, np.int64)
    recv = np.full(S, -1, np.int64)       # the spectators' watermark
    in_flight = np.full(S, -1, np.int64)  # the ack datagram built at the end of the previous call
    acked = np.full(S, -1, np.int64)      # what the host encodes against
    worst = 0
    for c in range(lost.shape[0]):
        newest[:] = (c + 1) * SPEC_CHUNK - 1 + TS.DELAY
        worst = max(worst, int((newest - acked).max()))
        stale = (recv >= 0) & (acked < recv - 2 * TS.W_)  # the reference is older than recv_inputs keeps: ignored
        arrived = ~lost[c, 0] & ~stale
        acked = np.where(lost[c, 1], acked, np.maximum(acked, in_flight))  # the previous call's ack arrives now
        recv = np.where(arrived, newest, recv)
        in_flight = recv.copy()
    assert worst > 3 * SPEC_CHUNK, "some acks arrive several calls late"
    assert fb * (worst + 6) + 3 <= row and worst + 6 + 1 <= R and 31 + 5 * 2 + row <= dg_row
    assert (recv > ticks - 8 * SPEC_CHUNK).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SPEC_RUNS))
def test_gpu_spectators_follow_their_host_over_datagrams(gpu_available, name):
    """P = 2, S = 70, rings on both sides.  Per call: the host ticks, exports its confirmed inputs,
    encodes both handles' frames into one packet per spectator endpoint (the spectator group), the
    packet rides an Input datagram that carries the host's connect status; a tenth of the datagrams
    is lost; the spectators parse, decode into their ring, take the host's status from the parse and
    tick on the lead's watermark row.  Their acks come back as InputAcks one call late (a tenth lost
    as well).  ex_game: player 1 is disconnected on the host at tick 100 (the truth run hands the oracle all of
    its inputs at once, fewer than its queue of 128).  The stub: 4-byte inputs,
    8-byte frames, both handles remote to the batch that decodes them.  After every call the
    spectators equal the truth run, what arrived equals what was exported, and no length or status
    is negative."""
    import torch

    import test_spectator as TS
    from test_delivery_ring import Feeder
    from test_p2p_pacing import dev
    game, mask, ticks, disc_t, row, dg_row = SPEC_RUNS[name]
    P, n = 2, S
    wide = game == G.Game.STUB
    raw = (lambda a: a.view(np.int32)) if wide else (lambda a: a)
    eg = G.EndpointGroups.spectator(P)
    lead = eg.lead_mask
    inputs, upto, rin = TS.host_network(game, P, mask, n, ticks + 8)
    host = TS.start_host(game, P, mask, n)
    spec = TS.start_spectators(game, P, n, catchup=2)
    host.set_delivery_ring(R)
    spec.set_delivery_ring(R)
    di, du = dev(raw(inputs), upto)
    fd = Feeder(P, mask, n, dtype=np.int32 if wide else np.uint8)
    feed = TS.Feed(host, R)
    tdt = torch.int32 if wide else torch.uint8
    out_ring, in_ring = G.DeliveryRing(R, P, n, dtype=tdt), G.DeliveryRing(R, P, n, dtype=tdt)
    out_ring.inputs = feed.inputs  # the host's export is the sender's ring
    seen = plain = TS.host_truth(game, P, mask, inputs, rin, ticks + 8)
    z = lambda shape, dt, v=0: torch.full(shape, v, dtype=dt, device="cuda")
    pk, ln, st = z((P, n, row), torch.uint8), z((P, n), torch.int32, SENT), z((P, n), torch.int32, SENT)
    dg, dl = z((2, P, n, dg_row), torch.uint8), z((2, P, n), torch.int32)
    adg, adl = z((2, P, n, 64), torch.uint8), z((2, P, n), torch.int32)
    cnt, bst = z((P, n), torch.int32), z((P, n), torch.int32)
    magic_host, magic_spec = z((P, n), torch.int16, 0x5A01), z((P, n), torch.int16, 0x5A02)
    no_ack, no_last, no_disc = z((P, n), torch.int32, -1), z((P, n), torch.int32, -1), z((P, n), torch.uint8)
    ones = z((P, n), torch.uint8, 1)
    heard_by_spec, heard_by_host = G.ParsedDatagrams(P, n, row), G.ParsedDatagrams(P, n, 32)
    acked = z((P, n), torch.int32, G.NULL_FRAME)
    lost = spectator_losses(ticks)
    status = z((P, n), torch.int32, SENT)
    sizes, disc_last = set(), None
    for c, t0 in enumerate(range(0, ticks, SPEC_CHUNK)):
        t1, now = t0 + SPEC_CHUNK, EPOCH_MS + TICK_MS * t0
        if t0 == disc_t:
            host.disconnect_player(1)
            disc_last = host.read_queues()[:, 1, 6].copy()
            seen = TS.host_truth(game, P, mask, inputs, rin, ticks + 8, disc=1, disc_last=disc_last)
        fd.feed(upto[t0:t1], raw(rin))
        host.run_ticks(di[t0:t1], du[t0:t1], fd.device())
        host.export_confirmed_inputs(feed.inputs, feed.upto, feed.last, feed.disc)
        newest = z((P, n), torch.int32, SENT)
        newest[0] = feed.upto
        out_ring.send_packets(None, newest, acked, 0, pk, ln, st, groups=eg)
        G.build_datagrams(lead, dg, dl, cnt, bst, magic_host, now, no_ack, feed.last, feed.disc, packets=pk, lengths=ln, start_frames=st)
        hl = ln.cpu().numpy()
        assert (hl[0] >= 0).all() and (hl[1] == SENT).all() and int(bst[0].abs().sum()) == 0, f"call {c}"
        sizes |= set(hl[0].tolist())
        # the host hears the acks the spectators built at the end of the previous call
        adl[0, 0, dev(lost[c, 1])] = 0
        G.parse_datagrams(heard_by_host, lead, adg, adl, magic_spec, now + FLIGHT_MS)
        next_acked = heard_by_host.acked.clone()
        # the network, then the spectators' side
        dl[0, 0, dev(lost[c, 0])] = 0
        G.parse_datagrams(heard_by_spec, lead, dg, dl, magic_host, now + FLIGHT_MS)
        in_ring.receive_packets(lead, heard_by_spec.packets, heard_by_spec.lengths, heard_by_spec.start_frames, TS.W_,
                                status=status, groups=eg)
        hs_ = status.cpu().numpy()
        assert (hs_[0] >= 0).all() and (hs_[1] == SENT).all() and int(heard_by_spec.status[0].sum()) == 0, f"call {c}"
        spec.receive_host_status(heard_by_spec.peer_last_frames[0].clone(), heard_by_spec.peer_disconnected[0].clone())
        assert torch.equal(in_ring.upto[0], in_ring.upto[1])
        spec.run_ticks(in_ring.upto[0][None].expand(t1 - t0, n).contiguous(), in_ring.inputs)
        TS.assert_state_is_truth(spec, seen, f"tick {t1 - 1}")
        got, sent_, to = in_ring.inputs.cpu().numpy(), feed.inputs.cpu().numpy(), in_ring.upto.cpu().numpy()
        for s in range(n):  # what arrived is what the host exported, frame by frame
            f = np.arange(max(0, to[0, s] - 30), to[0, s] + 1)
            np.testing.assert_array_equal(got[f & M, :, s], sent_[f & M, :, s], err_msg=f"tick {t1 - 1}, session {s}")
        G.build_datagrams(lead, adg, adl, cnt, bst, magic_spec, now + TICK_MS, in_ring.upto.clone(), no_last, no_disc, ack_owed=ones)
        acked = next_acked
    cur, _ = spec.frames()
    assert cur.min() > min(2 * R, ticks - 8 * SPEC_CHUNK) and spec.totals()[2] == 0
    assert (host.export_status()[0] == L.RB_P2P_EXPORT_OK).all() and max(sizes) > 32, "packets past the 32-byte head"
    if disc_t is not None:
        assert (cur > disc_last + 20).all(), "frames past the disconnect"
        changed = sum(not np.array_equal(seen[(s, int(cur[s]))][0], plain[(s, int(cur[s]))][0]) for s in range(n))
        assert changed > n // 2, "the disconnect changed the game the spectators show"
    for b in (host, spec):
        b.close()


# ---------------------------------------------------------------------------
# GPU 6: a 2-v-2 match over datagrams, one Input datagram per side and call
# ---------------------------------------------------------------------------
MATCH_T, MATCH_CUT_T, MATCH_SLOTS = 60, 12, 8  # (the slots of test_datagram.Wire)


def match_plan(n=S):
    """(lost [T, 2, slots, n] bool: the seeded tenth of the datagrams of either direction that never
    arrive; cut [n] bool: the pairs whose link is down for good from tick MATCH_CUT_T on)."""
    lost = np.random.default_rng(0x2B2).random((MATCH_T, 2, MATCH_SLOTS, n)) < 0.1
    cut = np.arange(n) % 9 == 4
    lost[MATCH_CUT_T:, :, :, cut] = True
    return lost, cut


def grouped_hop(wire, side, peer, back, eg, t, lost, what):
    """Tick t of one direction of the match: the sender's local handles are one group.  Export ->
    grouped encode -> build on the lead's row -> the losses -> parse -> grouped decode into the peer's
    ring, every step against the model; the ack the datagrams carry goes to the opposite sender."""
    import torch
    from test_p2p_pacing import dev
    from test_wire_ring import LOOP_D, LOOP_STRIDE
    link, P, n = wire.link, wire.P, wire.n
    lead, = eg.leads
    mem = list(eg.members(lead))
    far = wire.partner[lead]  # the lead of the peer's group: whose inputs this endpoint acknowledges
    now = EPOCH_MS + TICK_MS * t
    side.exported(link, what)
    assert torch.equal(link.sent[mem[0]], link.sent[mem[1]])
    acked, m_acked = link.acked()
    side.ring.send_packets(eg.lead_mask, link.sent, acked, LOOP_D, link.pk, link.ln, link.st, groups=eg)
    want = model_encode(side.m_ring, eg, m_acked, link.m_sent, LOOP_D, LOOP_STRIDE, True)
    ln, st, pk = (x.cpu().numpy() for x in (link.ln, link.st, link.pk))
    assert (want[1][lead] >= 0).all(), what
    np.testing.assert_array_equal(ln[lead], want[1][lead], err_msg=f"lengths, {what}")
    np.testing.assert_array_equal(st[lead], want[2][lead], err_msg=f"start frames, {what}")
    for (h, s), data in want[0].items():
        assert pk[h, s, :len(data)].tobytes() == data, f"packet ({h}, {s}), {what}"
    ack_frame = side.ring.upto[wire.partner].contiguous()
    m_ack = side.m_upto[far]
    G.build_datagrams(eg.lead_mask, wire.dg, wire.ln, wire.cnt, wire.st, wire.magic, now, ack_frame, wire.no_last, wire.no_disc,
                      packets=link.pk, lengths=link.ln, start_frames=link.st, ack_owed=wire.ones)
    count = wire.cnt.cpu().numpy()
    np.testing.assert_array_equal(count[lead], 1 + (want[1][lead] > 0), err_msg=f"an Input where frames are pending, and an InputAck, {what}")
    # the network
    through = ~lost & (np.arange(MATCH_SLOTS)[:, None] < count[lead][None, :])  # [slots, n]
    keep = np.zeros((MATCH_SLOTS, P, n), bool)
    keep[:, lead] = through
    wire.ln.mul_(dev(keep.astype(np.int32)))
    G.parse_datagrams(wire.parsed, eg.lead_mask, wire.dg, wire.ln, wire.magic, now + FLIGHT_MS)
    got = {k: v.cpu().numpy() for k, v in wire.parsed.tensors().items()}
    heard_input = through[0] & (want[1][lead] > 0)  # the Input is the endpoint's first datagram
    m_ln, m_st = np.zeros((P, n), np.int32), np.zeros((P, n), np.int32)
    m_pk = np.zeros((P, n, LOOP_STRIDE), np.uint8)
    m_ln[lead] = np.where(heard_input, want[1][lead], 0)
    m_st[lead] = np.where(heard_input, want[2][lead], 0)
    for (h, s), data in want[0].items():
        if heard_input[s]:
            m_pk[h, s, :len(data)] = np.frombuffer(data, np.uint8)
    wire.m_received[lead] = through.any(axis=0)
    wire.m_acked = np.where(through.any(axis=0), np.maximum(wire.m_acked, m_ack), wire.m_acked)  # both kinds carry the ack
    np.testing.assert_array_equal(got["received"][lead], wire.m_received[lead], err_msg=f"received, {what}")
    np.testing.assert_array_equal(got["lengths"][lead], m_ln[lead], err_msg=f"parsed lengths, {what}")
    np.testing.assert_array_equal(got["start_frames"][lead][heard_input], m_st[lead][heard_input], err_msg=f"parsed start frames, {what}")
    np.testing.assert_array_equal(got["acked"][lead], wire.m_acked, err_msg=f"parsed acks, {what}")
    assert not got["status"][lead].any() and not got["disconnect_requested"][lead].any(), what
    for s in np.nonzero(heard_input)[0]:
        assert got["packets"][lead, s, :m_ln[lead, s]].tobytes() == want[0][lead, s], f"parsed packet {s}, {what}"
    peer.ring.receive_packets(eg.lead_mask, wire.parsed.packets, wire.parsed.lengths, wire.parsed.start_frames, W,
                              status=link.status, groups=eg)
    m_status = np.full((P, n), SENT, np.int32)
    model_decode(peer.m_ring, peer.m_upto, m_status, eg, m_pk, m_ln, m_st, True)
    np.testing.assert_array_equal(link.status.cpu().numpy()[lead], m_status[lead], err_msg=f"decode status, {what}")
    np.testing.assert_array_equal(peer.ring.upto.cpu().numpy()[mem], peer.m_upto[mem], err_msg=f"upto, every member, {what}")
    assert (m_status[lead] >= 0).all(), what
    m_rows = np.full((P, n), -1, np.int32)
    m_rows[far] = wire.m_acked
    back.link.push(wire.parsed.acked[wire.partner].contiguous(), m_rows)  # what the opposite sender encodes against, 1-4 ticks on
    return int((m_status[lead] == 0).sum())


@pytest.mark.gpu
def test_gpu_a_two_against_two_match_over_datagrams(gpu_available):
    """Two ex_game batches of P = 4, each with two local handles: per call each exports its local
    inputs, encodes both handles' frames into ONE packet (groups {0,1} / {2,3}), builds one Input
    datagram (and an InputAck) on its lead's row; a tenth of the datagrams is lost; the peer parses,
    decodes the group into its ring, spreads the endpoint's `received` byte to both handles, polls
    liveness and ticks.  Acks travel in the datagrams and are used 1-4 ticks late.  After every call
    each batch equals the oracles and a twin fed the model's watermarks, the true inputs and the
    model's `received` bytes without any of this.  One pair in nine loses its link for good at tick
    12: liveness disconnects both of the peer's handles, at the same frame, on both sides."""
    import torch

    import test_liveness as TL
    import test_datagram
    from test_datagram import Wire
    from test_p2p_pacing import dev
    from test_wire_ring import Side
    assert test_datagram.MATCH_SLOTS == MATCH_SLOTS
    from ggrs_amd.synth import SEED
    P, n = 4, S
    masks = (0b0011, 0b1100)
    egs = [G.EndpointGroups([[0, 1]], P), G.EndpointGroups([[2, 3]], P)]
    X = G.synth_inputs(n, P, MATCH_T, seed=SEED ^ 0x2B2, mask=0x0F, dtype=np.uint8)
    lost, cut = match_plan()
    stream = torch.cuda.Stream()
    taken = 0
    with torch.cuda.stream(stream):
        sides = [Side(G.Game.EX_GAME, P, m, n, np.uint8, stream) for m in masks]
        models = [TL.Model(n, P, m, TL.NOTIFY, TL.TIMEOUT) for m in masks]
        for side in sides:
            for b in (side.sess, side.twin):
                b.enable_liveness(TL.TIMEOUT, TL.NOTIFY)
        wires = [Wire(P, m, n, 1, 0x5A00 + i) for i, m in enumerate(masks)]
        for w in wires:
            w.m_acked = np.full(n, -1, np.int32)
            w.m_received[:] = 0
        dx = dev(X)
        for t in range(MATCH_T):
            for i in (0, 1):
                taken += grouped_hop(wires[i], sides[i], sides[1 - i], wires[1 - i], egs[i], t, lost[t, i],
                                     f"hop {'AB'[i]} -> {'BA'[i]}, tick {t}")
            for i, side in enumerate(sides):
                peer, heard, eg = sides[1 - i], wires[1 - i], egs[1 - i]  # what the peer sent is what this side heard
                now, what = EPOCH_MS + TICK_MS * t, f"side {'AB'[i]}, tick {t}"
                received = eg.spread(heard.parsed.received)  # the endpoint's byte for every handle it carries
                requested = eg.spread(heard.parsed.disconnect_requested)
                m_received = eg.spread(heard.m_received.copy())
                before = side.cls.queues()[:, :, 7].T != 0
                newly, _ = models[i].poll(now, m_received, np.zeros((P, n), bool), side.cls.dead, before)
                for h in range(P):
                    if newly[h].any():
                        side.cls.disconnect(h, newly[h])
                np.testing.assert_array_equal(newly[eg.members(eg.leads[0])[0]], newly[eg.members(eg.leads[0])[1]], err_msg=what)
                side.sess.poll_liveness(now, received, requested)
                side.twin.poll_liveness(now, dev(m_received.astype(np.uint8)))
                side.tick(t, X, dx, lambda h: peer.truth[:, h], what)
                for x, y in zip(side.sess.read_liveness(), side.twin.read_liveness()):
                    assert np.array_equal(x, y), f"liveness, {what}"
                for got, want_, name in zip(side.sess.network_events(), models[i].event_arrays(), ("counts", "kinds", "handles", "values")):
                    np.testing.assert_array_equal(got, want_, err_msg=f"event {name}, {what}")
        assert taken > MATCH_T * n and cut.sum() >= 5
        for i, side in enumerate(sides):
            a, b = egs[1 - i].members(egs[1 - i].leads[0])
            q = side.sess.read_queues()
            assert q[cut][:, [a, b], 7].all() and not q[~cut][:, [a, b], 7].any(), "both handles of the silent peer, and nobody else"
            np.testing.assert_array_equal(q[:, a, 6], q[:, b, 6], err_msg="both handles end at the same frame")
            cur = side.sess.frames()[0]
            assert (cur[cut] > MATCH_T - 16).all() and (cur[~cut] > MATCH_T // 2).all() and side.sess.counters()[2] == 0
            kinds = side.sess.network_events()[1]
            assert (kinds[cut] == TL.DISCONNECTED).sum() == 2 * cut.sum() and not (kinds[~cut] == TL.DISCONNECTED).any()
        for s_ in sides:
            s_.close()
