"""GGRS's wire messages for every endpoint in one launch:
rb_parse_datagrams_all / rb_build_datagrams_all against a Python model.

The model packs and unpacks with `struct` from the wire table of include/ggrs_amd.h (bincode 1.3:
fixed-width little-endian integers, u32 variants, u64 Vec lengths, one-byte bools that must be 0 or
1, trailing bytes accepted) and restates UdpProtocol::handle_message / on_input / on_input_ack /
on_quality_report / on_quality_reply and the collecting half of on_checksum_report
(network/protocol.rs:544-722) in integers; nothing it expects comes from the code under test.
Every check is an equality.

Shapes: S = 70 (two waves, the second partly empty), P = 2, 3 and 4, M = 4 slots, stride 64 with
32-byte packet rows and stride 128 with 64-byte packet rows (payloads longer than the row).
"""
import ctypes
import functools
import os
import struct
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine library is loaded: the process then holds one HIP runtime, torch's)

import ggrs_amd as G
from ggrs_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "ggrs_amd", "csrc")
_TESTS = os.path.join(ROOT, "tests")

S, M, K = 70, 4, L.RB_P2P_REPORTS_PER_TAKE
GEOMS = {"short": (64, 32), "long": (128, 64)}   # datagram stride, packet stride
CASES = [(2, 0b10), (3, 0b101), (4, 0b1110), (4, 0b0101)]    # (P, handle mask)
CALLS = 12
EPOCH_MS = 1_700_000_000_000
NULL = -1
MASK64 = (1 << 64) - 1
MALFORMED, MISMATCH, SYNC_SEEN, BAD_PONG, DROPPED, NO_ROOM, ADV_RANGE = 1, 2, 4, 8, 16, 32, 64
KINDS = ["SyncRequest", "SyncReply", "Input", "InputAck", "QualityReport", "QualityReply", "ChecksumReport", "KeepAlive"]


def handles_of(mask, P):
    return [h for h in range(P) if (mask >> h) & 1]


# ---------------------------------------------------------------------------
# The model: the wire format
# ---------------------------------------------------------------------------
def head(magic, variant):
    return struct.pack("<HI", magic, variant)


def u128(v):
    return struct.pack("<QQ", v & MASK64, v >> 64)


def m_sync_request(magic, x):
    return head(magic, 0) + struct.pack("<I", x)


def m_sync_reply(magic, x):
    return head(magic, 1) + struct.pack("<I", x)


def m_input(magic, status, requested, start, ack, payload, n=None, length=None):
    """status: [(disconnected, last_frame)] per player; n / length override the two Vec lengths."""
    out = head(magic, 2) + struct.pack("<Q", len(status) if n is None else n)
    for d, lf in status:
        out += struct.pack("<Bi", d, lf)
    out += struct.pack("<Bii", requested, start, ack)
    return out + struct.pack("<Q", len(payload) if length is None else length) + payload


def m_input_ack(magic, ack):
    return head(magic, 3) + struct.pack("<i", ack)


def m_quality_report(magic, advantage, ping):
    return head(magic, 4) + struct.pack("<b", advantage) + u128(ping)


def m_quality_reply(magic, pong):
    return head(magic, 5) + u128(pong)


def m_checksum_report(magic, checksum, frame):
    return head(magic, 6) + u128(checksum) + struct.pack("<i", frame)


def m_keep_alive(magic):
    return head(magic, 7)


def payload_offset(P):
    return 31 + 5 * P


def input_boundaries(P, total):
    """Every byte count at which a truncated Input stops at a field boundary (or one byte short of its end)."""
    b = [0, 2, 6, 14]
    for i in range(P):
        b += [14 + 5 * i + 1, 14 + 5 * i + 5]
    r = 14 + 5 * P
    return sorted(set(b + [r + 1, r + 5, r + 9, r + 17, total - 1]))


class Short(Exception):
    pass


def unpack(data, P, why=None):
    """bincode::deserialize::<Message>(data) as a dict, or None where it fails; an Input whose
    status vector is not P long is refused too (the stated deviation).  why: a list that gets the
    reason of a refusal."""
    pos = 0

    def refuse(reason):
        if why is not None:
            why.append(reason)
        return None

    def take(fmt):
        nonlocal pos
        n = struct.calcsize(fmt)
        if pos + n > len(data):
            raise Short()
        v = struct.unpack_from(fmt, data, pos)
        pos += n
        return v[0] if len(v) == 1 else v

    def boolean():
        v = take("<B")
        if v > 1:
            raise Short("a bool of 2" if v == 2 else "a bool above 1")
        return v

    try:
        msg = {"magic": take("<H"), "kind": take("<I")}
        k = msg["kind"]
        if k > 7:
            return refuse("a variant of 8" if k == 8 else "a variant above 7")
        if k in (0, 1):
            msg["random"] = take("<I")
        elif k == 2:
            n = take("<Q")
            if n != P:
                return refuse("a Vec length of 2^63" if n == 1 << 63 else "a status vector of another length")
            msg["status"] = [(boolean(), take("<i")) for _ in range(n)]
            msg["requested"], msg["start"], msg["ack"] = boolean(), take("<i"), take("<i")
            length = take("<Q")
            if length > len(data) - pos:
                return refuse("a Vec length of 2^63" if length == 1 << 63 else "a length past the buffer")
            msg["payload"] = bytes(data[pos:pos + length])
        elif k == 3:
            msg["ack"] = take("<i")
        elif k == 4:
            msg["advantage"] = take("<b")
            lo, hi = take("<QQ")
            msg["ping"] = lo | (hi << 64)
        elif k == 5:
            lo, hi = take("<QQ")
            msg["pong"] = lo | (hi << 64)
        elif k == 6:
            lo, hi = take("<QQ")
            msg["checksum"], msg["frame"] = lo | (hi << 64), take("<i")
        return msg
    except Short as short:
        return refuse(str(short) or "truncated")


# ---------------------------------------------------------------------------
# The model: handle_message for one endpoint and one call
# ---------------------------------------------------------------------------
def fresh_state():
    return {"acked": NULL, "advantage": 0, "rtt": 0, "reports": []}


def model_parse(st, slots, magic, now, P, stride, packet_stride, seen=None):
    """slots: [(dg_length, row bytes)] in slot order.  Updates st (the in/out words and the kept
    reports) and returns the call's outputs."""
    out = {"received": 0, "requested": 0, "owed": 0, "ping": 0, "status": 0, "length": 0, "start": 0,
           "last": [NULL] * P, "disc": [0] * P, "packet": b""}
    inputs = 0
    for length, row in slots:
        if length <= 0:
            continue
        why = []
        msg = unpack(bytes(row[:min(length, stride)]), P, why)
        if msg is None:
            out["status"] |= MALFORMED
            if seen is not None:
                seen[why[0]] += 1
            continue
        if magic != 0 and msg["magic"] != magic:     # protocol.rs:551
            out["status"] |= MISMATCH
            continue
        out["received"] = 1                          # :555-556
        k = msg["kind"]
        if seen is not None:
            seen[KINDS[k]] += 1
            if magic == 0:
                seen["magic 0"] += 1
            if min(length, stride) > {0: 10, 1: 10, 3: 10, 4: 23, 5: 22, 6: 26, 7: 6}.get(k, payload_offset(P) + len(msg.get("payload", b""))):
                seen["trailing bytes accepted"] += 1
        if k == 2:                                   # on_input, :616-637
            inputs += 1
            if seen is not None and msg["ack"] < st["acked"]:
                seen["ack going backwards (Input)"] += 1
            st["acked"] = max(st["acked"], msg["ack"])
            if msg["requested"]:
                out["requested"] = 1
                if seen is not None and any(d or lf > out["last"][i] for i, (d, lf) in enumerate(msg["status"])):
                    seen["disconnect_requested with a status that must not be merged"] += 1
            else:
                for i, (d, lf) in enumerate(msg["status"]):
                    out["disc"][i] |= d
                    out["last"][i] = max(out["last"][i], lf)
            out["length"], out["start"] = len(msg["payload"]), msg["start"]
            out["packet"] = msg["payload"][:packet_stride]
            if seen is not None and len(msg["payload"]) > packet_stride:
                seen["payload longer than the packet row"] += 1
        elif k == 3:                                 # on_input_ack
            if seen is not None and msg["ack"] < st["acked"]:
                seen["ack going backwards (InputAck)"] += 1
            st["acked"] = max(st["acked"], msg["ack"])
        elif k == 4:                                 # on_quality_report, :697-701
            st["advantage"], out["owed"], out["ping"] = msg["advantage"], 1, msg["ping"]
        elif k == 5:                                 # on_quality_reply, :704-708
            if msg["pong"] > now or now - msg["pong"] > 0x7FFFFFFF:
                out["status"] |= BAD_PONG
                if seen is not None:
                    seen["pong in the future" if msg["pong"] >> 64 == 0 and msg["pong"] > now else
                         "pong with a non-zero high word" if msg["pong"] >> 64 else "round trip beyond int32"] += 1
            else:
                st["rtt"] = now - msg["pong"]
        elif k == 6:
            st["reports"].append((msg["checksum"], msg["frame"]))
        elif k in (0, 1):
            out["status"] |= SYNC_SEEN
    if len(st["reports"]) > K:
        if seen is not None and len(st["reports"]) == K + 1:
            seen["K + 1 checksum reports"] += 1
        st["reports"] = st["reports"][-K:]
        out["status"] |= DROPPED
    if seen is not None:
        seen["two Inputs in one call"] += inputs >= 2
        seen["an empty call"] += all(n <= 0 for n, _ in slots)
        seen["malformed"] += bool(out["status"] & MALFORMED)
        seen["magic mismatch"] += bool(out["status"] & MISMATCH)
    return out


# ---------------------------------------------------------------------------
# The seeded parse schedule
# ---------------------------------------------------------------------------
class Sched:
    pass


@functools.lru_cache(maxsize=None)
def schedule(P, geom):
    """CALLS calls over every endpoint (h, s): per call the clock, the `take` flag (the caller zeroes
    report_counts first) and M (dg_length, row) slots; rows are `stride` bytes, random past the datagram."""
    stride, packet_stride = GEOMS[geom]
    rng = np.random.default_rng(0xD6 + 16 * P + (geom == "long"))
    off = payload_offset(P)
    sc = Sched()
    sc.P, sc.stride, sc.packet_stride = P, stride, packet_stride
    sc.magic = np.array([[0 if s % 5 == 0 else 0x1000 + 256 * h + s for s in range(S)] for h in range(P)], np.uint16)
    sc.now = [EPOCH_MS + 16 * c for c in range(CALLS)]
    sc.take = [c % 4 == 0 for c in range(CALLS)]
    sc.truncated_at = set()
    ri = lambda lo, hi: int(rng.integers(lo, hi))

    def status():
        return [(ri(0, 2), ri(-1, 500)) for _ in range(P)]

    def pay(n=None):
        return rng.integers(0, 256, ri(1, min(stride - off, 24) + 1) if n is None else n, dtype=np.uint8).tobytes()

    def slots_of(k, c, h, s):
        good = int(sc.magic[h, s]) or 0x4242
        bad = good ^ 0x0101
        now, a = sc.now[c], 10 * c + ri(0, 8)
        if k == 0:
            return []
        if k == 1:
            return [m_input(good, status(), 0, a, a - 1, pay()), m_quality_report(good, ri(-128, 128), now - 3),
                    m_keep_alive(good), m_input_ack(good, a + 2)]
        if k == 2:
            return [m_sync_request(good, ri(0, 1 << 32)), m_sync_reply(good, ri(0, 1 << 32)),
                    m_quality_reply(good, now - ri(0, 400)), m_checksum_report(good, ri(0, 1 << 62) << 66 | ri(0, 1 << 62), 10 * c)]
        if k == 3:
            return [m_input(good, status(), 0, a, a + 3, pay()), m_input(good, status(), 0, a + 1, a, pay()),
                    m_input_ack(good, a - 2)]
        if k == 4:
            return [m_input(good, [(0, ri(0, 50)) for _ in range(P)], 0, a, a, pay()),
                    m_input(good, [(1, 1000 + i) for i in range(P)], 1, a + 1, a + 1, pay())]
        if k == 5:
            return [m_keep_alive(bad), m_input(bad, status(), 1, a, a + 50, pay()), m_input(good, status(), 0, a, a, pay())]
        if k == 6:
            full = m_input(good, status(), 0, a, a, pay())
            bounds = input_boundaries(P, len(full))
            cut = bounds[(s + c + h) % len(bounds)]
            sc.truncated_at.add((cut if cut != len(full) - 1 else "end - 1"))
            return [full[:cut], m_input_ack(good, a)] if cut else [(0, b""), m_input_ack(good, a)]
        if k == 7:
            st = status()
            i = ri(0, P + 1)
            if i < P:
                st[i] = (2, st[i][1])
            return [m_input(good, st, 2 if i == P else 0, a, a + 9, pay()), m_quality_report(good, 5, now)]
        if k == 8:
            return [head(good, 8) + bytes(8), head(good, 0xFFFFFFFF) + bytes(20), m_keep_alive(good)]
        if k == 9:
            return [m_input(good, status(), 0, a, a + 9, pay(), n=1 << 63), m_input(good, status(), 0, a, a + 9, pay(), length=1 << 63),
                    m_input(good, status(), 0, a, a + 9, pay(5), length=6), m_input(good, status(), 0, a, a + 9, pay(), length=(1 << 32) + 1)]
        if k == 10:
            return [m_input_ack(good, a) + b"\x01\x02\x03", m_keep_alive(good) + bytes(ri(1, 40)),
                    m_input(good, status(), 0, a, a, pay(4)) + b"\xff\xff", m_quality_reply(good, now - 7) + b"\x09"]
        if k == 11:
            return [m_input(good, status(), 0, a, a, pay(stride - off))]
        if k == 12:
            return [m_checksum_report(good, (c << 70) | (3 * c + j), 100 * c + j) for j in range(3)] + [m_keep_alive(good)]
        if k == 13:
            return [m_quality_reply(good, now + 5), m_quality_reply(good, (1 << 64) | 5), m_quality_reply(good, 0),
                    m_quality_reply(good, now - 123)]
        if k == 14:  # a length beyond the stride (the row ends first), a negative one over garbage
            return [(1000, m_keep_alive(good)), (-5, m_input_ack(good, 9999)), (stride + 1, m_input(good, status(), 0, a, a, pay(stride - off))),
                    (2 * stride, m_input(good, status(), 0, a, a, pay(3), length=stride))]
        return [m_quality_report(good, -128, 1 << 100), m_quality_report(good, 127, (7 << 64) | c), m_input_ack(good, -1)]

    sc.calls = []
    for c in range(CALLS):
        call = []
        for h in range(P):
            per = []
            for s in range(S):
                k = 12 if s % 10 == 3 else (5 * s + 3 * c + 7 * h) % 16
                rows = []
                for item in slots_of(k, c, h, s):
                    n, data = item if isinstance(item, tuple) else (len(item), item)
                    assert len(data) <= stride, (k, len(data))
                    row = rng.integers(0, 256, stride, dtype=np.uint8)
                    row[:len(data)] = np.frombuffer(data, np.uint8)
                    rows.append((n, row.tobytes()))
                rows += [(0, rng.integers(0, 256, stride, dtype=np.uint8).tobytes())] * (M - len(rows))
                per.append(rows[:M])
            call.append(per)
        sc.calls.append(call)
    return sc


def run_model(sc, seen=None):
    """Per call [h][s] -> (outputs, in/out words after the call, kept reports after the call)."""
    P = sc.P
    st = [[fresh_state() for _ in range(S)] for _ in range(P)]
    res = []
    for c in range(CALLS):
        call = []
        for h in range(P):
            row = []
            for s in range(S):
                if sc.take[c]:
                    st[h][s]["reports"] = []
                out = model_parse(st[h][s], sc.calls[c][h][s], int(sc.magic[h, s]), sc.now[c], P, sc.stride, sc.packet_stride, seen)
                row.append((out, st[h][s]["acked"], st[h][s]["advantage"], st[h][s]["rtt"], list(st[h][s]["reports"])))
            call.append(row)
        res.append(call)
    return res


# ---------------------------------------------------------------------------
# The model: the messages an endpoint owes, and the seeded build cases
# ---------------------------------------------------------------------------
def model_build(o, P, slots, stride, packet_stride, seen=None):
    """o: the endpoint's owed fields.  Returns (datagrams, status)."""
    out, status = [], 0

    def room(n):
        nonlocal status
        if len(out) < slots and n <= stride:
            return True
        status |= NO_ROOM
        if seen is not None:
            seen["build overflowing M_out" if len(out) >= slots else "build overflowing stride"] += 1
        return False

    length = o["length"]
    if length > packet_stride:
        status |= MALFORMED
        length = 0
    if length > 0 and room(payload_offset(P) + length):
        out.append(m_input(o["magic"], list(zip(o["disc"], o["last"])), o["requested"], o["start"], o["ack"], o["packet"][:length]))
    if o["ack_owed"] and room(10):
        out.append(m_input_ack(o["magic"], o["ack"]))
    if o["reply_owed"] and room(22):
        out.append(m_quality_reply(o["magic"], o["ping"]))
    if o["report_due"]:
        if not -128 <= o["advantage"] <= 127:
            status |= ADV_RANGE
        elif room(23):
            out.append(m_quality_report(o["magic"], o["advantage"], o["now"]))
    for checksum, frame in o["reports"]:
        if frame != NULL and room(26):
            out.append(m_checksum_report(o["magic"], checksum, frame))
    if o["keepalive"]:
        if not out and room(6):
            out.append(m_keep_alive(o["magic"]))
        elif seen is not None and out:
            seen["a KeepAlive suppressed by another message"] += 1
    return out, status


@functools.lru_cache(maxsize=None)
def build_cases(P, geom):
    stride, packet_stride = GEOMS[geom]
    rng = np.random.default_rng(0xB1 + 16 * P + (geom == "long"))
    ri = lambda lo, hi: int(rng.integers(lo, hi))
    cases = []
    for h in range(P):
        row = []
        for s in range(S):
            k = (s + 3 * h) % 10
            reports = [(0, NULL)] * K                      # one tensor per session: the same for every handle
            srng = np.random.default_rng(1000 + s)
            n_rep = {4: K, 7: 2}.get(s % 10, 0)
            for j in sorted(srng.choice(K, n_rep, replace=False)):
                reports[j] = (int(srng.integers(0, 1 << 62)) << 64 | int(srng.integers(0, 1 << 62)), int(srng.integers(0, 900)))
            o = {"magic": ri(1, 1 << 16), "now": EPOCH_MS + s, "length": 0, "start": ri(0, 400), "ack": ri(-1, 400),
                 "requested": 0, "last": [ri(-1, 400) for _ in range(P)], "disc": [ri(0, 2) for _ in range(P)],
                 "ack_owed": 0, "reply_owed": 0, "ping": ri(0, 1 << 62) << 64 | ri(0, 1 << 62), "report_due": 0,
                 "advantage": ri(-128, 128), "keepalive": 0, "reports": reports,
                 "packet": rng.integers(0, 256, packet_stride, dtype=np.uint8).tobytes()}
            fits = stride - payload_offset(P)
            if k == 0:
                o["length"] = -1 - (s % 2)                  # the encoder's refusals: no Input
            elif k == 1:
                o["keepalive"] = 1
            elif k == 2:
                o["keepalive"] = o["ack_owed"] = 1
            elif k == 3:
                o["length"] = ri(1, min(fits, packet_stride) + 1)
            elif k == 4:
                o.update(length=ri(1, min(fits, packet_stride) + 1), ack_owed=1, reply_owed=1, report_due=1, keepalive=1)
            elif k == 5:
                o.update(length=packet_stride - ri(0, 4), ack_owed=1)   # short geometry: longer than the stride takes
            elif k == 6:
                o.update(report_due=1, advantage=[200, -129, 128, 1 << 20][s % 4], reply_owed=1)
            elif k == 7:
                o.update(report_due=1, advantage=[-128, 127, 0][s % 3])
            elif k == 8:
                o.update(length=min(fits, packet_stride), requested=1, ack_owed=1, reply_owed=1)
            else:
                o.update(length=packet_stride + 1 + (s % 3) * 1000, keepalive=1)
            row.append(o)
        cases.append(row)
    return cases


# ---------------------------------------------------------------------------
# CPU 1-4
# ---------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "ggrs_amd.h")).read()
    lib = L.load()
    for name in ("rb_parse_datagrams_all", "rb_build_datagrams_all"):
        assert f"rb_status {name}(" in header
        assert hasattr(lib, name) and name in [n for n, _, _ in L.SIGNATURES]
    for bit, value in [("RB_DG_MALFORMED", 1), ("RB_DG_MAGIC_MISMATCH", 2), ("RB_DG_SYNC_SEEN", 4), ("RB_DG_BAD_PONG", 8),
                       ("RB_DG_REPORTS_DROPPED", 16), ("RB_DG_NO_ROOM", 32), ("RB_DG_ADVANTAGE_RANGE", 64)]:
        assert f"#define {bit} {value} " in header and getattr(L, bit) == value
    for cited in ("protocol.rs:544-575", "udp_socket.rs:31-45", "protocol.rs:468-525", ":627-636", ":706"):
        assert cited in header, cited
    # the structs as ctypes lays them out are the header's: pointer, int64 and paired int32 fields only
    assert ctypes.sizeof(L.RbDatagramParse) == 8 * 22 and ctypes.sizeof(L.RbDatagramBuild) == 8 * 23
    assert "RB_PLUGIN_ABI 8" in open(os.path.join(ROOT, "include", "ggrs_amd_game.hpp")).read()
    assert callable(G.parse_datagrams) and callable(G.build_datagrams)


def test_known_answer_datagrams():
    assert m_keep_alive(0x1234) == bytes.fromhex("341207000000")
    assert m_input_ack(0x1234, 5) == bytes.fromhex("34120300000005000000")
    assert m_quality_report(0x1234, -2, 1000) == bytes.fromhex("341204000000fee803") + bytes(14)
    assert unpack(m_keep_alive(0x1234), 2) == {"magic": 0x1234, "kind": 7}
    assert unpack(m_input_ack(0x1234, 5) + b"\x00", 2)["ack"] == 5
    assert unpack(m_quality_report(0x1234, -2, 1000), 2) == {"magic": 0x1234, "kind": 4, "advantage": -2, "ping": 1000}
    msg = m_input(0x1234, [(0, 7), (1, -1)], 0, 8, 6, b"\x02\x09")
    assert len(msg) == payload_offset(2) + 2 and unpack(msg, 2)["payload"] == b"\x02\x09" and unpack(msg, 4) is None
    assert unpack(msg[:-1], 2) is None and unpack(msg + b"\x00", 2)["status"] == [(0, 7), (1, -1)]


@functools.lru_cache(maxsize=None)
def check_program():
    import tempfile
    exe = os.path.join(tempfile.mkdtemp(prefix="check_datagram_"), "check_datagram")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", _CSRC, "-o", exe,
                    os.path.join(_TESTS, "check_datagram.cpp")], check=True)
    return exe


def hexof(b):
    return b.hex() if b else "-"


@pytest.mark.parametrize("P,geom", [(2, "short"), (3, "short"), (4, "short"), (2, "long"), (3, "long"), (4, "long")])
def test_the_parse_step_on_the_host_equals_the_model(tmp_path, P, geom):
    """tests/check_datagram.cpp drives datagram_step.hpp, the functions the kernel calls, over every
    endpoint of the schedule, each datagram in a buffer of exactly its bytes."""
    sc = schedule(P, geom)
    lines = [f"{P} {P * S} {M} {sc.stride} {sc.packet_stride} {CALLS}", " ".join(str(int(x)) for x in sc.magic.reshape(-1))]
    for c in range(CALLS):
        lines.append(f"{sc.now[c]} {int(sc.take[c])}")
        for h in range(P):
            for s in range(S):
                lines.append(" ".join(f"{n} {hexof(row[:min(n, sc.stride)]) if n > 0 else '-'}" for n, row in sc.calls[c][h][s]))
    path = tmp_path / "parse.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([check_program(), "parse", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    want = []
    for c, call in enumerate(run_model(sc)):
        for h in range(P):
            for s in range(S):
                o, acked, adv, rtt, reports = call[h][s]
                line = (f"{c} {h * S + s} {o['received']} {o['requested']} {acked} {adv} {rtt} {o['owed']} {o['ping'] & MASK64} "
                        f"{o['ping'] >> 64} {o['status']} {o['length']} {o['start']} {len(reports)} | "
                        + " ".join(str(x) for x in o["last"] + o["disc"]) + f" | {hexof(o['packet'])} |"
                        + "".join(f" {cs & MASK64} {cs >> 64} {fr}" for cs, fr in reports))
                want.append(line)
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


def build_line(o, P):
    return (f"{o['magic']} {o['now']} {o['length']} {o['start']} {o['ack']} {o['requested']} " + " ".join(str(x) for x in o["last"] + o["disc"])
            + f" {o['ack_owed']} {o['reply_owed']} {o['ping'] & MASK64} {o['ping'] >> 64} {o['report_due']} {o['advantage']} {o['keepalive']} "
            + " ".join(f"{cs & MASK64} {cs >> 64} {fr}" for cs, fr in o["reports"]) + " ")


@pytest.mark.parametrize("P,geom", [(2, "short"), (3, "short"), (4, "short"), (2, "long"), (3, "long"), (4, "long")])
def test_the_build_step_on_the_host_equals_the_model(tmp_path, P, geom):
    stride, packet_stride = GEOMS[geom]
    cases = [o for row in build_cases(P, geom) for o in row]
    lines = [f"{P} {M} {stride} {packet_stride} {len(cases)}"]
    for o in cases:
        lines.append(build_line(o, P) + (hexof(o["packet"][:o["length"]]) if 0 < o["length"] <= packet_stride else "-"))
    path = tmp_path / "build.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([check_program(), "build", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    got = r.stdout.splitlines()
    assert len(got) == len(cases)
    for i, o in enumerate(cases):
        msgs, status = model_build(o, P, M, stride, packet_stride)
        assert got[i] == f"{i} {len(msgs)} {status}" + "".join(f" {len(m)} {m.hex()}" for m in msgs), i


def test_the_schedules_show_every_situation():
    """The witness, on the model alone: every situation the issue lists occurs at least once."""
    from collections import Counter
    for P in (2, 3, 4):
        seen = Counter()
        for geom in GEOMS:
            sc = schedule(P, geom)
            run_model(sc, seen)
            total = payload_offset(P) + 8
            want = {("end - 1" if b == total - 1 else b) for b in input_boundaries(P, total)} - {0}
            assert {b for b in sc.truncated_at if b != 0} >= {b for b in want if b != "end - 1"} and "end - 1" in sc.truncated_at
            for row in build_cases(P, geom):
                for o in row:
                    model_build(o, P, M, *GEOMS[geom], seen)
        # direct witnesses of the malformed kinds: each is refused by unpack for its own reason
        good = m_input(7, [(0, 1)] * P, 0, 3, 2, b"abc")
        assert unpack(good, P) is not None
        two = bytearray(good)
        two[14] = 2
        assert unpack(bytes(two), P) is None                                       # a bool of 2
        assert unpack(head(7, 8) + bytes(8), P) is None                             # a variant of 8
        assert unpack(m_input(7, [(0, 1)] * P, 0, 3, 2, b"abc", length=1 << 63), P) is None   # a Vec length of 2^63
        assert unpack(m_input(7, [(0, 1)] * P, 0, 3, 2, b"abc", n=1 << 63), P) is None
        for name in KINDS + ["two Inputs in one call", "ack going backwards (Input)", "ack going backwards (InputAck)",
                             "disconnect_requested with a status that must not be merged", "magic mismatch", "magic 0",
                             "malformed", "truncated", "a bool of 2", "a variant of 8", "a Vec length of 2^63",
                             "a length past the buffer", "trailing bytes accepted", "payload longer than the packet row",
                             "K + 1 checksum reports", "pong in the future", "pong with a non-zero high word",
                             "round trip beyond int32", "an empty call", "build overflowing M_out",
                             "build overflowing stride", "a KeepAlive suppressed by another message"]:
            assert seen[name] > 0, (P, name)


# ---------------------------------------------------------------------------
# GPU helpers: tensors between guard regions
# ---------------------------------------------------------------------------
GUARD = 256
SENT = 0xA5  # what guards, and rows nobody may write, are prefilled with


def guarded(shape, dtype, fill=None):
    """(buffer, view): a tensor of `shape` between two GUARD-byte regions of SENT, itself SENT-filled or `fill`."""
    import torch
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    pad = (-n) % 16
    buf = torch.full((GUARD + n + pad + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    view = buf[GUARD:GUARD + n].view(dtype).view(shape)
    if fill is not None:
        view.fill_(fill)
    return buf, view


def guards_intact(buf, n):
    b = buf.cpu().numpy()
    return (b[:GUARD] == SENT).all() and (b[GUARD + n:] == SENT).all()


class GuardedParse:
    """A ParsedDatagrams whose every tensor sits between guards, prefilled with SENT bytes except the
    in/out words, which start as the model's."""

    def __init__(self, P, packet_stride):
        import torch
        self.out = G.ParsedDatagrams(P, S, packet_stride)
        self.bufs = {}
        for name, t in self.out.tensors().items():
            buf, view = guarded(tuple(t.shape), t.dtype)
            if name in ("acked", "frame_advantage", "rtt_ms", "report_counts"):
                view.copy_(t)
            self.bufs[name] = (buf, view.numel() * view.element_size())
            setattr(self.out, name, view)
        self.before = {k: v.cpu().numpy().copy() for k, v in self.out.tensors().items()}

    def host(self):
        return {k: v.cpu().numpy() for k, v in self.out.tensors().items()}

    def intact(self):
        return all(guards_intact(buf, n) for buf, n in self.bufs.values())


def report_words(reports):
    """[(checksum, frame)] -> int64 [K, 3] in rb_checksum_report's layout, cleared past the list."""
    w = np.zeros((K, 3), np.uint64)
    w[:, 2] = MASK64
    for j, (cs, fr) in enumerate(reports):
        w[j] = (cs & MASK64, cs >> 64, (fr & 0xFFFFFFFF) | (0xFFFFFFFF << 32))
    return w.view(np.int64)


def datagram_tensors(sc, c):
    import torch
    P = sc.P
    rows = np.zeros((M, P, S, sc.stride), np.uint8)
    lens = np.zeros((M, P, S), np.int32)
    for h in range(P):
        for s in range(S):
            for m, (n, row) in enumerate(sc.calls[c][h][s]):
                rows[m, h, s] = np.frombuffer(row, np.uint8)
                lens[m, h, s] = n
    return torch.from_numpy(rows).cuda(), torch.from_numpy(lens).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("P,mask", CASES)
def test_gpu_parse_equals_the_model_inside_guards(gpu_available, P, mask, geom):
    """Every call of the schedule, the in/out tensors carried from call to call: every output of
    every endpoint served equals the model's, rows of other handles keep their prefill, guards stay."""
    import torch
    sc = schedule(P, geom)
    model = run_model(sc)
    gp = GuardedParse(P, sc.packet_stride)
    out = gp.out
    magic = torch.from_numpy(sc.magic.view(np.int16)).cuda()
    hs = handles_of(mask, P)
    others = [h for h in range(P) if h not in hs]
    for c in range(CALLS):
        if sc.take[c]:
            out.report_counts[hs] = 0
        dg, ln = datagram_tensors(sc, c)
        keep = (dg.clone(), ln.clone())
        G.parse_datagrams(out, mask, dg, ln, magic, sc.now[c])
        got = gp.host()
        assert torch.equal(dg, keep[0]) and torch.equal(ln, keep[1])
        for h in hs:
            for s in range(S):
                o, acked, adv, rtt, reports = model[c][h][s]
                what = f"call {c}, endpoint ({h}, {s})"
                assert (got["received"][h, s], got["disconnect_requested"][h, s], got["reply_owed"][h, s]) == \
                    (o["received"], o["requested"], o["owed"]), what
                assert (got["acked"][h, s], got["frame_advantage"][h, s], got["rtt_ms"][h, s]) == (acked, adv, rtt), what
                assert (int(got["reply_ping"][0, h, s]) & MASK64, int(got["reply_ping"][1, h, s]) & MASK64) == \
                    (o["ping"] & MASK64, o["ping"] >> 64), what
                assert got["status"][h, s] == o["status"], what
                assert (got["lengths"][h, s], got["start_frames"][h, s]) == (o["length"], o["start"]), what
                assert got["peer_last_frames"][h, :, s].tolist() == o["last"], what
                assert got["peer_disconnected"][h, :, s].tolist() == o["disc"], what
                assert got["packets"][h, s, :len(o["packet"])].tobytes() == o["packet"], what
                assert got["report_counts"][h, s] == len(reports), what
                assert np.array_equal(got["reports"][h, :, s], report_words(reports)), what
        for name, t in got.items():
            rows = t[:, others] if name == "reply_ping" else t[others]
            want = gp.before[name][:, others] if name == "reply_ping" else gp.before[name][others]
            assert np.array_equal(rows, want), f"{name}: rows outside the mask, call {c}"
        assert gp.intact(), f"guards, call {c}"


def build_tensors(cases, P, packet_stride):
    import torch
    a = lambda f, dt: torch.from_numpy(np.array([[f(o) for o in row] for row in cases], dt)).cuda()
    t = {
        "local_magic": a(lambda o: o["magic"], np.uint16).view(torch.int16),
        "ack_frame": a(lambda o: o["ack"], np.int32),
        "lengths": a(lambda o: o["length"], np.int32),
        "start_frames": a(lambda o: o["start"], np.int32),
        "disconnect_requested": a(lambda o: o["requested"], np.uint8),
        "ack_owed": a(lambda o: o["ack_owed"], np.uint8),
        "reply_owed": a(lambda o: o["reply_owed"], np.uint8),
        "report_due": a(lambda o: o["report_due"], np.uint8),
        "keepalive_due": a(lambda o: 3 * o["keepalive"], np.uint8),
        "frame_advantage": a(lambda o: o["advantage"], np.int32),
    }
    ping = np.array([[[o["ping"] & MASK64 for o in row] for row in cases], [[o["ping"] >> 64 for o in row] for row in cases]], np.uint64)
    t["reply_ping"] = torch.from_numpy(ping.view(np.int64)).cuda()
    pk = np.array([[np.frombuffer(o["packet"], np.uint8) for o in row] for row in cases], np.uint8)
    t["packets"] = torch.from_numpy(pk).cuda()
    relaid = np.zeros((K, S, 3), np.int64)
    for s in range(S):   # the take tensor keeps a report in its own entry: gaps stay where they are
        w = np.zeros((K, 3), np.uint64)
        w[:, 2] = MASK64
        for j, (cs, fr) in enumerate(cases[0][s]["reports"]):
            if fr != NULL:
                w[j] = (cs & MASK64, cs >> 64, (fr & 0xFFFFFFFF) | (0xFFFFFFFF << 32))
        relaid[:, s] = w.view(np.int64)
    t["reports"] = torch.from_numpy(relaid).cuda()
    return t


def session_status(cases, P):
    """The sender's connect status is per session: handle 0's row of the cases serves every endpoint."""
    import torch
    last = np.array([[cases[0][s]["last"][i] for s in range(S)] for i in range(P)], np.int32)
    disc = np.array([[cases[0][s]["disc"][i] for s in range(S)] for i in range(P)], np.uint8)
    return torch.from_numpy(last).cuda(), torch.from_numpy(disc).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("P,mask", CASES)
def test_gpu_build_equals_the_models_bytes_inside_guards(gpu_available, P, mask, geom):
    import torch
    stride, packet_stride = GEOMS[geom]
    cases = [[dict(o, last=build_cases(P, geom)[0][s]["last"], disc=build_cases(P, geom)[0][s]["disc"],
                   reports=build_cases(P, geom)[0][s]["reports"]) for s, o in enumerate(row)] for row in build_cases(P, geom)]
    t = build_tensors(cases, P, packet_stride)
    last, disc = session_status(cases, P)
    bufs = {}
    outs = {}
    for name, shape, dt in [("dg", (M, P, S, stride), torch.uint8), ("ln", (M, P, S), torch.int32), ("cnt", (P, S), torch.int32),
                            ("st", (P, S), torch.int32)]:
        buf, view = guarded(shape, dt)
        bufs[name], outs[name] = (buf, view.numel() * view.element_size()), view
    before = {k: v.cpu().numpy().copy() for k, v in outs.items()}
    now = EPOCH_MS + 99
    G.build_datagrams(mask, outs["dg"], outs["ln"], outs["cnt"], outs["st"], t["local_magic"], now, t["ack_frame"], last, disc,
                      packets=t["packets"], lengths=t["lengths"], start_frames=t["start_frames"],
                      disconnect_requested=t["disconnect_requested"], ack_owed=t["ack_owed"], reply_owed=t["reply_owed"],
                      reply_ping=t["reply_ping"], report_due=t["report_due"], frame_advantage=t["frame_advantage"],
                      reports=t["reports"], keepalive_due=t["keepalive_due"])
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    hs = handles_of(mask, P)
    for h in hs:
        for s in range(S):
            msgs, status = model_build(dict(cases[h][s], now=now), P, M, stride, packet_stride)
            what = f"endpoint ({h}, {s})"
            assert (got["cnt"][h, s], got["st"][h, s]) == (len(msgs), status), what
            assert got["ln"][:, h, s].tolist() == [len(m) for m in msgs] + [0] * (M - len(msgs)), what
            for k, m in enumerate(msgs):
                assert got["dg"][k, h, s, :len(m)].tobytes() == m, f"{what}, datagram {k}"
    others = [h for h in range(P) if h not in hs]
    for name in got:
        a, b = (got[name][:, others], before[name][:, others]) if name in ("dg", "ln") else (got[name][others], before[name][others])
        assert np.array_equal(a, b), f"{name}: rows outside the mask"
    assert all(guards_intact(buf, n) for buf, n in bufs.values())
    # the optional tensors left out: nothing is due but what the required ones say (nothing)
    for v in outs.values():
        v.fill_(SENT)
    G.build_datagrams(mask, outs["dg"], outs["ln"], outs["cnt"], outs["st"], t["local_magic"], now, t["ack_frame"], last, disc)
    assert (outs["cnt"][hs] == 0).all() and (outs["ln"][:, hs] == 0).all() and (outs["st"][hs] == 0).all()
    assert (outs["dg"] == SENT).all()


@pytest.mark.gpu
@pytest.mark.parametrize("P", [2, 4])
def test_gpu_build_then_parse_returns_the_fields(gpu_available, P):
    """Random field values through build and back through parse: every field arrives as it left."""
    import torch
    stride, packet_stride = GEOMS["long"]
    rng = np.random.default_rng(0x707 + P)
    mask = (1 << P) - 1
    dev = lambda a: torch.from_numpy(a).cuda()
    magic = rng.integers(1, 1 << 16, (P, S)).astype(np.uint16)
    ack = rng.integers(-1, 1 << 30, (P, S)).astype(np.int32)
    start = rng.integers(0, 1 << 30, (P, S)).astype(np.int32)
    lengths = rng.integers(1, packet_stride + 1, (P, S)).astype(np.int32)
    packets = rng.integers(0, 256, (P, S, packet_stride)).astype(np.uint8)
    requested = (rng.random((P, S)) < 0.3).astype(np.uint8)
    last = rng.integers(-1, 1 << 30, (P, S)).astype(np.int32)
    disc = rng.integers(0, 2, (P, S)).astype(np.uint8)
    sent_at, recv_at = EPOCH_MS, EPOCH_MS + 37
    ping = np.zeros((2, P, S), np.int64)                    # the pongs: most in the past, some not
    ping[0] = recv_at - rng.integers(0, 5000, (P, S))
    ping[0][:, ::5] += 6000
    ping[1][:, ::7] = rng.integers(1, 1 << 62, (P, S))[:, ::7]
    adv = rng.integers(-128, 128, (P, S)).astype(np.int32)
    ones = torch.ones((P, S), dtype=torch.uint8, device="cuda")
    dg = torch.zeros((M, P, S, stride), dtype=torch.uint8, device="cuda")
    ln = torch.zeros((M, P, S), dtype=torch.int32, device="cuda")
    cnt, st = (torch.zeros((P, S), dtype=torch.int32, device="cuda") for _ in range(2))
    G.build_datagrams(mask, dg, ln, cnt, st, dev(magic.view(np.int16)), sent_at, dev(ack), dev(last), dev(disc),
                      packets=dev(packets), lengths=dev(lengths), start_frames=dev(start), disconnect_requested=dev(requested),
                      ack_owed=ones, reply_owed=ones, reply_ping=dev(ping), report_due=ones, frame_advantage=dev(adv))
    assert (cnt == 4).all() and (st == 0).all()
    out = G.ParsedDatagrams(P, S, packet_stride)
    G.parse_datagrams(out, mask, dg, ln, dev(magic.view(np.int16)), recv_at)
    got = {k: v.cpu().numpy() for k, v in out.tensors().items()}
    assert (got["received"] == 1).all() and (got["reply_owed"] == 1).all()
    assert np.array_equal(got["acked"], np.maximum(ack, -1)) and np.array_equal(got["disconnect_requested"], requested)
    assert np.array_equal(got["lengths"], lengths) and np.array_equal(got["start_frames"], start)
    assert np.array_equal(got["frame_advantage"], adv) and (got["reply_ping"][0] == sent_at).all() and (got["reply_ping"][1] == 0).all()
    for h in range(P):
        merged = requested[h] == 0
        assert np.array_equal(got["peer_last_frames"][h][:, merged], last[:, merged])
        assert np.array_equal(got["peer_disconnected"][h][:, merged], disc[:, merged])
        assert (got["peer_last_frames"][h][:, ~merged] == NULL).all() and (got["peer_disconnected"][h][:, ~merged] == 0).all()
        for s in range(S):
            assert np.array_equal(got["packets"][h, s, :lengths[h, s]], packets[h, s, :lengths[h, s]])
    # the echoed pong comes back as a round-trip time: the QualityReply carried reply_ping's low word
    ok = (ping[1] == 0) & (ping[0] <= recv_at)
    assert ok.any() and (~ok).any() and np.array_equal(got["status"], np.where(ok, 0, BAD_PONG))
    assert np.array_equal(got["rtt_ms"][ok], (recv_at - ping[0][ok]).astype(np.int32)) and (got["rtt_ms"][~ok] == 0).all()
    assert (got["report_counts"] == 0).all() and (got["reports"][..., 2] == -1).all()


@pytest.mark.gpu
def test_gpu_invalid_requests_leave_every_tensor_as_it_was(gpu_available):
    import torch
    P, (stride, packet_stride) = 2, GEOMS["short"]
    sc = schedule(P, "short")
    dg, ln = datagram_tensors(sc, 1)
    magic = torch.from_numpy(sc.magic.view(np.int16)).cuda()
    gp = GuardedParse(P, packet_stride)

    def parse(mask=0b11, datagrams=dg, lengths=ln, now=EPOCH_MS, players=None):
        if players is None:
            return G.parse_datagrams(gp.out, mask, datagrams, lengths, magic, now)
        lib, out = L.load(), gp.out
        io = L.RbDatagramParse(**{k: ctypes.c_void_p(v.data_ptr()) for k, v in out.tensors().items()},
                               datagrams=ctypes.c_void_p(datagrams.data_ptr()), stride=stride, slots=M,
                               dg_lengths=ctypes.c_void_p(lengths.data_ptr()), remote_magic=ctypes.c_void_p(magic.data_ptr()),
                               now_ms=now, packet_stride=packet_stride)
        return lib.rb_parse_datagrams_all(0, None, mask, players, S, ctypes.byref(io))

    wide = torch.zeros((M, P, S, 72), dtype=torch.uint8, device="cuda")        # not a multiple of 16
    narrow = torch.zeros((M, P, S, 48), dtype=torch.uint8, device="cuda")      # below 64
    many = torch.zeros((9, P, S, stride), dtype=torch.uint8, device="cuda")    # M out of range
    odd = torch.zeros((M * P * S * stride + 16,), dtype=torch.uint8, device="cuda")[8:8 + M * P * S * stride].view(M, P, S, stride)
    for kw in [dict(mask=0), dict(mask=0b100), dict(datagrams=wide), dict(datagrams=narrow), dict(datagrams=odd), dict(now=-1),
               dict(datagrams=many, lengths=torch.zeros((9, P, S), dtype=torch.int32, device="cuda"))]:
        with pytest.raises(G.InvalidRequest):
            parse(**kw)
    assert parse(mask=0b11111, players=5) == L.RB_INVALID_REQUEST     # P > 4
    assert parse(mask=0b1, players=0) == L.RB_INVALID_REQUEST
    torch.cuda.synchronize()
    for k, v in gp.host().items():
        assert np.array_equal(v, gp.before[k]), k
    assert gp.intact()

    cases = build_cases(P, "short")
    t = build_tensors(cases, P, packet_stride)
    last, disc = session_status(cases, P)
    outs = {"dg": torch.full((M, P, S, stride), SENT, dtype=torch.uint8, device="cuda"),
            "ln": torch.full((M, P, S), 7, dtype=torch.int32, device="cuda"),
            "cnt": torch.full((P, S), 7, dtype=torch.int32, device="cuda"), "st": torch.full((P, S), 7, dtype=torch.int32, device="cuda")}
    keep = {k: v.clone() for k, v in outs.items()}

    def build(mask=0b11, out=None, lens=None, now=EPOCH_MS, packets=t["packets"]):
        G.build_datagrams(mask, outs["dg"] if out is None else out, outs["ln"] if lens is None else lens, outs["cnt"], outs["st"],
                          t["local_magic"], now, t["ack_frame"], last, disc, packets=packets, lengths=t["lengths"],
                          start_frames=t["start_frames"], keepalive_due=t["keepalive_due"])

    thin = torch.zeros((P, S, 24), dtype=torch.uint8, device="cuda")            # a packet row no encoder writes
    for kw in [dict(mask=0), dict(mask=0b1000), dict(out=wide), dict(out=narrow), dict(out=odd), dict(now=-5), dict(packets=thin),
               dict(out=many, lens=torch.zeros((9, P, S), dtype=torch.int32, device="cuda"))]:
        with pytest.raises(G.InvalidRequest):
            build(**kw)
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert torch.equal(v, keep[k]), k
    assert not wide.any() and not narrow.any() and not many.any() and not odd.any()


# ---------------------------------------------------------------------------
# GPU 5, 6: two batches play each other over datagrams only
# ---------------------------------------------------------------------------
MATCH_STRIDE = 192     # 31 + 5 P + a 128-byte packet row, in whole 16-byte chunks
MATCH_SLOTS = 8        # Input, InputAck, QualityReply, QualityReport and the tick's ChecksumReports all fit
TICK_MS = 16
FLIGHT_MS = 3          # a datagram is parsed this long after it was built
QUALITY_EVERY = 12     # ticks between two QualityReports


class Wire:
    """One direction of a match: the sender's Link (tests/test_wire_ring.py: its packets, `sent`, the
    acks as they came back 1-4 ticks late) with the datagram layer on top, on the device and in the model."""

    def __init__(self, P, mask, n, ib, magic):
        from test_wire_ring import LOOP_STRIDE, Link
        self.link = Link(P, mask, n, ib)
        self.P, self.mask, self.n = P, mask, n
        self.hs = handles_of(mask, P)
        self.partner = [(h + P // 2) % P for h in range(P)]     # row h acks the inputs of handle partner[h]
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        self.dg, self.ln = z((MATCH_SLOTS, P, n, MATCH_STRIDE), torch.uint8), z((MATCH_SLOTS, P, n), torch.int32)
        self.cnt, self.st = z((P, n), torch.int32), z((P, n), torch.int32)
        self.magic = torch.full((P, n), magic, dtype=torch.int16, device="cuda")
        self.m_magic = magic
        self.ones = torch.ones((P, n), dtype=torch.uint8, device="cuda")
        self.no_last = torch.full((P, n), NULL, dtype=torch.int32, device="cuda")
        self.no_disc = z((P, n), torch.uint8)
        self.parsed = G.ParsedDatagrams(P, n, LOOP_STRIDE)
        # the model's side of what the parse returns, per endpoint row
        self.m_state = [[fresh_state() for _ in range(n)] for _ in range(P)]
        self.m_received = np.zeros((P, n), np.uint8)
        self.m_owed = np.zeros((P, n), np.uint8)
        self.m_ping = np.zeros((P, n), np.uint64)
        self.m_last = np.full((P, P, n), NULL, np.int32)
        self.m_disc = np.zeros((P, P, n), np.uint8)


class Owed:
    """What a side owes its peer besides inputs and acks (the full match): its connect status, the
    tick's checksum reports and its frame advantage, on the device (from the batch) and in the model
    (from the oracles and the time-sync model)."""

    def __init__(self, side):
        from test_wire_ring import R
        P, n = side.P, side.n
        self.side = side
        self.ring = torch.zeros((R, P, n), dtype=torch.uint8, device="cuda")
        self.upto = torch.full((n,), NULL, dtype=torch.int32, device="cuda")
        self.last = torch.full((P, n), NULL, dtype=torch.int32, device="cuda")
        self.disc = torch.zeros((P, n), dtype=torch.uint8, device="cuda")
        self.adv = torch.zeros((P, n), dtype=torch.int32, device="cuda")
        self.reports = None
        self.m_adv = np.zeros((P, n), np.int32)
        self.gather()

    def gather(self):
        side = self.side
        side.sess.export_confirmed_inputs(self.ring, self.upto, self.last, self.disc)
        q = side.cls.queues()
        self.m_last, self.m_disc = q[:, :, 6].T.astype(np.int32), q[:, :, 7].T.astype(np.uint8)
        self.reports = side.sess.take_checksum_reports()
        side.twin.take_checksum_reports()
        self.m_reports = [None] * side.n
        for orc, k in zip(side.cls.orcs, side.cls.cols):
            fr, cs = orc.take_checksum_reports(K)
            for j, s in enumerate(k):
                self.m_reports[s] = [((int(cs[e, j, 1]) << 64) | int(cs[e, j, 0]), int(fr[e, j])) for e in range(K)]
        side.sess.export_time_sync(local_adv=self.adv)
        self.m_adv = side.model.state()["local_adv"]


def datagram_hop(wire, side, peer, back, t, lost, swapped, what, owed=None):
    """Tick t of one direction: export and encode as tests/test_wire_ring.py does, then build -> the
    seeded loss and slot swaps -> parse -> decode into the peer's ring; every tensor against the models.
    back: the opposite Wire, whose sender learns its acks from what this hop's parse returns and whose
    parse says which QualityReply this sender owes.  owed: the sender's Owed in the full match."""
    from test_wire_ring import LOOP_D, LOOP_STRIDE, SENT as RING_SENT, W, model_decode, model_encode
    link, P, n, hs, pt = wire.link, wire.P, wire.n, wire.hs, wire.partner
    now = EPOCH_MS + TICK_MS * t
    side.exported(link, what)
    acked, m_acked = link.acked()
    side.ring.send_packets(link.mask, link.sent, acked, LOOP_D, link.pk, link.ln, link.st)
    want = model_encode(side.m_ring, link.mask, m_acked, link.m_sent, LOOP_D, LOOP_STRIDE)
    assert (want[1][hs] >= 0).all(), what
    # the sender acknowledges what its own ring holds of the partner handle's inputs
    ack_frame = side.ring.upto[pt].contiguous()
    m_ack = side.m_upto[pt]
    due = owed is not None and t % QUALITY_EVERY == 0
    if owed is None:
        G.build_datagrams(link.mask, wire.dg, wire.ln, wire.cnt, wire.st, wire.magic, now, ack_frame, wire.no_last, wire.no_disc,
                          packets=link.pk, lengths=link.ln, start_frames=link.st, ack_owed=wire.ones, keepalive_due=wire.ones)
    else:
        G.build_datagrams(link.mask, wire.dg, wire.ln, wire.cnt, wire.st, wire.magic, now, ack_frame, owed.last, owed.disc,
                          packets=link.pk, lengths=link.ln, start_frames=link.st, ack_owed=wire.ones, keepalive_due=wire.ones,
                          reply_owed=back.parsed.reply_owed[pt].contiguous(), reply_ping=back.parsed.reply_ping[:, pt].contiguous(),
                          report_due=wire.ones if due else None, frame_advantage=owed.adv[pt].contiguous() if due else None,
                          reports=owed.reports)
    dg, ln = wire.dg.cpu().numpy(), wire.ln.cpu().numpy()
    sent = {}
    for h in hs:
        for s in range(n):
            o = {"magic": wire.m_magic, "now": now, "length": int(want[1][h, s]), "start": int(want[2][h, s]), "ack": int(m_ack[h, s]),
                 "requested": 0, "last": [NULL] * P, "disc": [0] * P, "ack_owed": 1, "reply_owed": 0, "ping": 0, "report_due": 0,
                 "advantage": 0, "keepalive": 1, "reports": [], "packet": want[0].get((h, s), b"")}
            if owed is not None:
                o.update(last=owed.m_last[:, s].tolist(), disc=owed.m_disc[:, s].tolist(), reply_owed=int(back.m_owed[pt[h], s]),
                         ping=int(back.m_ping[pt[h], s]), report_due=int(due), advantage=int(owed.m_adv[pt[h], s]),
                         reports=owed.m_reports[s])
            msgs, status = model_build(o, P, MATCH_SLOTS, MATCH_STRIDE, LOOP_STRIDE)
            assert status == 0 and ln[:, h, s].tolist() == [len(m) for m in msgs] + [0] * (MATCH_SLOTS - len(msgs)), f"{what}, ({h}, {s})"
            for k, m in enumerate(msgs):
                assert dg[k, h, s, :len(m)].tobytes() == m, f"{what}, ({h}, {s}), datagram {k}"
            sent[h, s] = msgs
    # the network: a tenth of the datagrams lost, the first two slots swapped now and then
    keep = ~lost
    order = np.arange(MATCH_SLOTS)[:, None, None].repeat(P, 1).repeat(n, 2)
    order[0][swapped], order[1][swapped] = 1, 0
    idx = torch.from_numpy(order).cuda()
    wire.dg.copy_(torch.gather(wire.dg, 0, idx[..., None].expand(-1, -1, -1, MATCH_STRIDE)))
    wire.ln.copy_(torch.gather(wire.ln, 0, idx) * torch.from_numpy(keep.astype(np.int32)).cuda())
    heard_at = now + FLIGHT_MS
    G.parse_datagrams(wire.parsed, link.mask, wire.dg, wire.ln, wire.magic, heard_at)
    got = {k: v.cpu().numpy() for k, v in wire.parsed.tensors().items()}
    m_pk = np.zeros((P, n, LOOP_STRIDE), np.uint8)
    m_ln, m_st = np.zeros((P, n), np.int32), np.zeros((P, n), np.int32)
    m_acked = np.full((P, n), NULL, np.int32)
    for h in hs:
        for s in range(n):
            msgs = sent[h, s] + [b""] * (MATCH_SLOTS - len(sent[h, s]))
            slots = [(len(msgs[order[m, h, s]]) * int(keep[m, h, s]), msgs[order[m, h, s]]) for m in range(MATCH_SLOTS)]
            st = wire.m_state[h][s]
            o = model_parse(st, slots, wire.m_magic, heard_at, P, MATCH_STRIDE, LOOP_STRIDE)
            where = f"{what}, ({h}, {s})"
            assert (got["received"][h, s], got["status"][h, s], got["lengths"][h, s], got["start_frames"][h, s]) == \
                (o["received"], o["status"], o["length"], o["start"]), where
            assert got["acked"][h, s] == st["acked"], where
            assert got["packets"][h, s, :o["length"]].tobytes() == o["packet"], where
            assert got["peer_last_frames"][h, :, s].tolist() == o["last"] and got["peer_disconnected"][h, :, s].tolist() == o["disc"], where
            assert (got["frame_advantage"][h, s], got["rtt_ms"][h, s], got["reply_owed"][h, s]) == (st["advantage"], st["rtt"], o["owed"]), where
            assert (int(got["reply_ping"][0, h, s]), int(got["reply_ping"][1, h, s])) == (o["ping"] & MASK64, o["ping"] >> 64), where
            assert got["report_counts"][h, s] == len(st["reports"]) and np.array_equal(got["reports"][h, :, s], report_words(st["reports"])), where
            m_pk[h, s, :o["length"]] = np.frombuffer(o["packet"], np.uint8)
            m_ln[h, s], m_st[h, s], m_acked[h, s] = o["length"], o["start"], st["acked"]
            wire.m_received[h, s], wire.m_owed[h, s], wire.m_ping[h, s] = o["received"], o["owed"], o["ping"] & MASK64
            wire.m_last[h, :, s], wire.m_disc[h, :, s] = o["last"], o["disc"]
    peer.ring.receive_packets(link.mask, wire.parsed.packets, wire.parsed.lengths, wire.parsed.start_frames, W, status=link.status)
    m_status = np.full((P, n), RING_SENT, np.int32)
    model_decode(peer.m_ring, peer.m_upto, m_status, link.mask, m_pk, m_ln, m_st)
    np.testing.assert_array_equal(link.status.cpu().numpy()[hs], m_status[hs], err_msg=f"decode status, {what}")
    np.testing.assert_array_equal(peer.ring.upto.cpu().numpy()[hs], peer.m_upto[hs], err_msg=f"upto, {what}")
    assert (m_status[hs] >= 0).all(), what
    # the acks this hop carried are what the opposite sender encodes against, 1-4 ticks from now
    back.link.push(wire.parsed.acked[pt].contiguous(), m_acked[pt])
    return int(lost[:, hs].sum()), int(swapped[hs].sum())


def hand_over(side, heard):
    """The full match: what the parse of `heard` (the peer's Wire) returned goes into the side's
    batch from the parse's tensors, and into its twin, its oracles and its time-sync model from the
    model's values.  Returns the number of checksum reports handed over."""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n, handed = side.n, 0
    for h in heard.hs:
        states = heard.m_state[h]
        side.sess.receive_peer_connect_status(h, heard.parsed.peer_last_frames[h], heard.parsed.peer_disconnected[h])
        side.twin.receive_peer_connect_status(h, dev(heard.m_last[h]), dev(heard.m_disc[h]))
        side.sess.receive_checksum_reports(h, heard.parsed.reports[h])
        side.twin.receive_checksum_reports(h, dev(np.stack([report_words(st["reports"]) for st in states], axis=1)))
        fr = np.full((K, n), NULL, np.int32)
        cs = np.zeros((K, n, 2), np.uint64)
        for s, st in enumerate(states):
            for j, (c, f) in enumerate(st["reports"]):
                fr[j, s], cs[j, s] = f, (c & MASK64, c >> 64)
            handed += len(st["reports"])
            st["reports"] = []
        for orc, k in zip(side.cls.orcs, side.cls.cols):
            orc.receive_peer_connect_status(h, heard.m_last[h][:, k], heard.m_disc[h][:, k])
            orc.receive_checksum_reports(h, fr[:, k], cs[:, k])
        rtt = np.array([st["rtt"] for st in states], np.int32)
        adv = np.array([st["advantage"] for st in states], np.int32)
        side.sess.receive_quality(h, heard.parsed.rtt_ms[h], heard.parsed.frame_advantage[h])
        side.twin.receive_quality(h, dev(rtt), dev(adv))
        side.model.receive_quality(h, rtt, adv)
    heard.parsed.report_counts[heard.hs] = 0      # the slices were taken
    return handed


# The stub games sum exactly two inputs (two players only), so "P = 4 with the stub's 4-byte inputs"
# is two matches: four players (ex_game, two local handles a side) and 4-byte inputs (the stub, P = 2).
# name: game, input dtype, input mask, P, calls, full (peer status, desync detection and time sync on and in the datagrams)
MATCHES = {"exgame-p2-full": (G.Game.EX_GAME, np.uint8, 0x0F, 2, 150, True), "exgame-p4": (G.Game.EX_GAME, np.uint8, 0x0F, 4, 60, False),
           "stub-u32-p2": (G.Game.STUB, np.uint32, 0xFFFFFFFF, 2, 60, False)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MATCHES))
def test_gpu_two_batches_play_each_other_over_datagrams_only(gpu_available, name):
    """Two batches, each local to half the handles, one tick per call: local-input export -> encode ->
    build -> (a tenth of the datagrams lost, two slots swapped now and then) -> parse -> decode into
    the ring -> liveness poll -> tick, the acks travelling in the datagrams and used 1-4 ticks late.
    After every call each batch equals the oracles and a twin fed the model's watermarks, the true
    inputs and the model's `received` bytes directly, without the datagram layer.
    The full match (ex_game, P = 2, 150 calls) runs with peers' connect status, desync detection and
    time sync on, and the datagrams carry them: every Input has the sender's connect status
    (rb_p2p_export_confirmed_inputs' rows -> peer_last_frames -> receive_peer_connect_status), the
    tick's checksum reports travel as ChecksumReports (take -> build -> parse -> reports / report_counts
    -> receive_checksum_reports), and every 12 ticks a QualityReport carries export_time_sync's
    local_adv, answered by a QualityReply (frame_advantage / rtt_ms -> receive_quality).  The twin,
    the oracles and the time-sync model get the model's values of the same messages."""
    from test_p2p_pacing import dev
    from test_time_sync import make_session
    from test_wire_ring import LOOP_D, R, SL, Side
    from ggrs_amd.synth import SEED
    game, dtype, imask, P, ticks, full = MATCHES[name]
    half = (1 << (P // 2)) - 1
    masks = (half, half << (P // 2))
    X = G.synth_inputs(SL, P, ticks, seed=SEED ^ 0xD6, mask=imask, dtype=dtype)
    rng = np.random.default_rng(0xD6D6)
    lost = rng.random((ticks, 2, MATCH_SLOTS, P, SL)) < 0.1
    swapped = rng.random((ticks, 2, P, SL)) < 0.15
    stream = torch.cuda.Stream()
    n_lost = n_swapped = handed = 0
    with torch.cuda.stream(stream):
        sides = [Side(game, P, m, SL, dtype, stream, time_sync=full, desync=10 if full else 0) for m in masks]
        for side in sides:
            if full:  # the same batches with peers' connect status on
                for name_ in ("sess", "twin"):
                    getattr(side, name_).close()
                    b = make_session(game, P, side.mask, LOOP_D, LOOP_D, sessions=SL, time_sync=True, desync=10, peer=True)
                    b.set_stream(stream)
                    b.set_delivery_ring(R)
                    setattr(side, name_, b)
            for b in (side.sess, side.twin):
                b.enable_liveness()
        wires = [Wire(P, m, SL, np.dtype(dtype).itemsize, 0x5A00 + i) for i, m in enumerate(masks)]
        owed = [Owed(side) if full else None for side in sides]
        dx = dev(X.view(np.int32) if dtype == np.uint32 else X)
        for t in range(ticks):
            for i in (0, 1):
                a, b = datagram_hop(wires[i], sides[i], sides[1 - i], wires[1 - i], t, lost[t, i], swapped[t, i],
                                    f"hop {'AB'[i]} -> {'BA'[i]}, tick {t}", owed[i])
                n_lost, n_swapped = n_lost + a, n_swapped + b
            for i, side in enumerate(sides):
                peer, heard = sides[1 - i], wires[1 - i]      # what the peer sent is what this side heard
                now = EPOCH_MS + TICK_MS * t
                if full:
                    handed += hand_over(side, heard)
                side.sess.poll_liveness(now, heard.parsed.received, heard.parsed.disconnect_requested)
                side.twin.poll_liveness(now, torch.from_numpy(heard.m_received).cuda())
                side.tick(t, X, dx, lambda h: peer.truth[:, h], f"side {'AB'[i]}, tick {t}")
                for x, y in zip(side.sess.read_liveness(), side.twin.read_liveness()):
                    assert np.array_equal(x, y), f"liveness, side {'AB'[i]}, tick {t}"
                if full:
                    ev, tw = side.sess.desync_events(), side.twin.desync_events()
                    for x, y in zip(ev, tw):
                        assert np.array_equal(x, y), f"desync events against the twin, side {'AB'[i]}, tick {t}"
                    want = side.cls.gather([o.desync_events()[0] for o in side.cls.orcs], 0)
                    assert np.array_equal(ev[0], want), f"desync events against the oracles, side {'AB'[i]}, tick {t}"
                    owed[i].gather()
        assert n_lost > ticks * SL // 10 and n_swapped > ticks
        assert all((s.sess.frames()[0] > ticks // 2).all() for s in sides) and all(s.sess.counters()[2] == 0 for s in sides)
        assert all(s.sess.network_events()[0].sum() == 0 for s in sides)
        if full:
            assert handed > 2 * SL * (ticks // 10 - 3), "checksum reports crossed the wire all match long"
            for s in sides:
                fa, la, ra, rtt = s.sess.read_time_sync()
                assert (ra != 0).any() and (rtt != 0).any(), "quality messages reached the batch"
        for s in sides:
            s.close()
