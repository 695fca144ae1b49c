"""rb_endpoint_protocol_poll_all: UdpProtocol's sync handshake, state machine
and send timers for every endpoint of a batch in one launch.

Every check is an equality.  What an endpoint must do comes from the model below, which restates the
cited lines of the reference's network/protocol.rs in Python integers, with the set of outstanding
nonces bounded to the newest 8; what a sync datagram must hold comes from the struct helpers
test_datagram.py writes its messages with.  Nothing comes from the code under test.

The schedule is seeded and adaptive: a scripted peer per endpoint reads the model's state to answer
(or withhold, repeat, corrupt) the nonces the endpoint sent.  Its clock steps 16 +- 5 ms: twelve
seeded steps that sum to 200 ms repeat through the first part, so a stamp set in call a is read at
exactly stamp + 200 in call a + 12; after one 300 ms gap twelve steps that sum to 201 ms repeat, so
there it is read at stamp + 201; then one gap above 5000 ms.  No 5000 ms boundary can be met across
a gap above 5000 ms, and with both stamps set together the quality report always goes before a
KeepAlive, so those situations arrive as state rows the caller writes (load_state_dict's way in).
"""
import collections
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

S, M, STRIDE, K = 70, 4, 64, L.RB_P2P_REPORTS_PER_TAKE
GEOMS = [(2, 4), (3, 2), (4, 4), (2, 2)]                      # (P, sync_slots)
CASES = [(2, 4, 0b10), (2, 2, 0b01), (2, 4, 0b11), (3, 2, 0b101), (3, 2, 0b010), (3, 2, 0b111), (4, 4, 0b1110), (4, 4, 0b0101),
         (4, 4, 0b1111)]  # (P, sync_slots, handle mask)
CALLS = 130
GAP_300, GAP_5000 = 40, 80   # the calls the two gaps precede
EPOCH_MS = 1_700_000_000_000
NULL = -1
INIT, SYNCING, RUNNING, DISCONNECTED, SHUTDOWN = range(5)
NO_ROOM = 32
EV_SYNCHRONIZING, EV_SYNCHRONIZED = 1, 2
SEED = 20


def handles_of(mask, P):
    return [h for h in range(P) if (mask >> h) & 1]


# ---------------------------------------------------------------------------
# The wire format of the two sync kinds (test_datagram.py's helpers)
# ---------------------------------------------------------------------------
def head(magic, variant):
    return struct.pack("<HI", magic, variant)


def m_sync_request(magic, x):
    return head(magic, 0) + struct.pack("<I", x)


def m_sync_reply(magic, x):
    return head(magic, 1) + struct.pack("<I", x)


# ---------------------------------------------------------------------------
# The model: network/protocol.rs over integers
# ---------------------------------------------------------------------------
def fresh():
    return {"state": INIT, "remaining": 0, "nonces": [0] * 8, "valid": 0, "next": 0, "last_send": 0, "last_input_recv": 0,
            "last_quality_report": 0, "shutdown_at": 0, "stats_start": 0, "sent": 0, "last_newest": 0, "remote_magic": 0}


def blank_out():
    return {"input_length": 0, "ack_due": 0, "reply_due": 0, "report_due": 0, "keepalive_due": 0, "msgs": [], "events": 0,
            "sync_count": 0, "liveness": 1, "queue": 0, "synchronized": 1, "status": 0}


def model_step(st, i, sync_slots, seen=None):
    """One endpoint, one call; `st` is updated in place.  i: now, magic, start, disconnected, ack_owed,
    reply_owed, received, newest, acked, length, reports, slots [(n, bytes)], nonces [M]."""
    seen = collections.Counter() if seen is None else seen
    out = blank_out()
    if st["state"] >= SHUTDOWN:   # send_all_messages :429-432, handle_message :546-548
        if any(n >= 10 and bytes(b[2:6]) == bytes(4) for n, b in i["slots"]):
            seen["request unanswered in Shutdown"] += 1
        return out
    now = i["now"]
    used = [0]          # the caller's nonces consumed
    due = [0]           # messages queued apart from the sync ones: queue_message :527-538
    state0 = st["state"]

    def timer(name, stamp, delay):
        if now == stamp + delay:
            seen[f"{name}: now == stamp + delay, nothing fires"] += 1
        if now == stamp + delay + 1:
            seen[f"{name}: now == stamp + delay + 1 fires"] += 1
        return stamp + delay < now

    def last_send():    # queue_message stamps last_send_time at once, :533
        return now if len(out["msgs"]) + due[0] > 0 else st["last_send"]

    def queue_sync(data):
        if len(out["msgs"]) >= sync_slots:
            out["status"] |= NO_ROOM
            seen["more sync messages than sync_slots"] += 1
            return False
        out["msgs"].append(data)
        return True

    def send_sync_request():   # :507-514
        if used[0] >= len(i["nonces"]):
            out["status"] |= NO_ROOM
            return
        x = i["nonces"][used[0]]
        if not queue_sync(m_sync_request(i["magic"], x)):
            return
        used[0] += 1
        held = [k for k in range(8) if (st["valid"] >> k) & 1 and st["nonces"][k] == x]
        if held:
            seen["a duplicate nonce from the caller"] += 1
            return
        at = st["next"] & 7
        if (st["valid"] >> at) & 1:
            seen["an outstanding nonce evicted"] += 1
            st.setdefault("evicted", []).append(st["nonces"][at])
        st["nonces"][at] = x
        st["valid"] |= 1 << at
        st["next"] = (at + 1) & 7

    if i["disconnected"] and st["state"] != DISCONNECTED:   # disconnect(), :325-333
        seen[f"disconnected in state {st['state']}"] += 1
        st["state"] = DISCONNECTED
        st["shutdown_at"] = now + 5000
    if i["start"] and st["state"] == INIT:                  # synchronize(), :335-341
        st["state"] = SYNCING
        st["remaining"] = 5
        st["stats_start"] = now
        st["last_send"] = st["last_input_recv"] = st["last_quality_report"] = now
        send_sync_request()
    good = 0
    for n, data in i["slots"]:                               # handle_message, :544-575
        n = min(n, STRIDE)
        if n == 9 and bytes(data[2:6]) in (bytes(4), b"\x01\x00\x00\x00"):
            seen["a truncated 9-byte sync datagram"] += 1
        if n < 10:
            continue
        magic, variant, x = struct.unpack("<HII", bytes(data[:10]))
        if variant > 1:
            continue
        if st["remote_magic"] != 0 and magic != st["remote_magic"]:   # :551
            seen["magic filter drops a sync message"] += 1
            if st.get("magic_set_in_call") == i["call"]:
                seen["magic filter with the magic an earlier slot of the call set"] += 1
            continue
        if variant == 0:                                     # on_sync_request, :578-583
            if queue_sync(m_sync_reply(i["magic"], x)):
                seen[f"request answered in state {st['state']}"] += 1
            continue
        if st["state"] != SYNCING:                           # on_sync_reply, :586-614
            if st["state"] == RUNNING:
                seen["a reply after Running" if good == 0 or st.get("magic_set_in_call") != i["call"] else
                     "the fifth good reply followed by another in the same call"] += 1
            continue
        hit = [k for k in range(8) if (st["valid"] >> k) & 1 and st["nonces"][k] == x]
        if not hit:
            seen["a reply to an evicted nonce" if x in st.get("evicted", []) else "a reply with an unknown nonce"] += 1
            continue
        for k in hit:
            st["valid"] &= ~(1 << k)
        good += 1
        if good == 2:
            seen["two good replies in one call"] += 1
        st["remaining"] -= 1
        if st["remaining"] > 0:
            out["events"] |= EV_SYNCHRONIZING
            send_sync_request()
        else:
            st["state"] = RUNNING
            out["events"] |= EV_SYNCHRONIZED
            st["remote_magic"] = magic
            st["magic_set_in_call"] = i["call"]
            seen["handshake finished" + (" after a retry" if st.get("retried") else " in five round trips")] += 1
    if i["ack_owed"]:                                        # :654, :682
        out["ack_due"] = 1
        st["last_input_recv"] = now
        due[0] += 1
    if i["reply_owed"]:                                      # :697-701
        out["reply_due"] = 1
        due[0] += 1
    input_due = shut = False
    if st["state"] == SYNCING:                               # poll, :351-404
        if timer("sync retry", last_send(), 200):
            st["retried"] = True
            send_sync_request()
    elif st["state"] == RUNNING:
        if timer("resend", st["last_input_recv"], 200):
            st["last_input_recv"] = now
            input_due = i["newest"] > i["acked"]
            seen["resend with pending output" if input_due else "resend with none: the stamp resets, no Input"] += 1
            if input_due and st.get("held_back") == i["newest"]:
                seen["an input of the Synchronizing time leaves by the resend timer"] += 1
        if timer("quality report", st["last_quality_report"], 200):
            st["last_quality_report"] = now
            out["report_due"] = 1
            due[0] += 1
    elif st["state"] == DISCONNECTED:
        if timer("shutdown", st["shutdown_at"], 0):
            st["state"] = SHUTDOWN
            shut = True
    newest1 = 0 if i["newest"] < 0 else i["newest"] + 1
    if newest1 > st["last_newest"]:                          # send_input, :444-446
        if st["state"] == RUNNING:
            input_due = True
        else:
            st["held_back"] = i["newest"]
            seen[f"a new input in state {st['state']} is not sent"] += 1
        st["last_newest"] = newest1
    elif st["state"] == RUNNING and st.get("held_back") == i["newest"] and not input_due and state0 != RUNNING:
        seen["an input held back is not sent late once Running"] += 1
    if input_due:
        out["input_length"] = i["length"]
        due[0] += 1
    due[0] += i["reports"]                                   # :736-742
    if st["state"] == RUNNING and timer("keep-alive", st["last_send"], 200):   # :372-375
        kinds = [k for k, on in (("sync message", out["msgs"]), ("InputAck", out["ack_due"]), ("QualityReply", out["reply_due"]),
                                 ("QualityReport", out["report_due"]), ("Input", input_due), ("ChecksumReport", i["reports"])) if on]
        if kinds:
            for k in kinds if len(kinds) == 1 else []:
                seen[f"keep-alive suppressed by {k} alone"] += 1
        else:
            out["keepalive_due"] = 1
            due[0] += 1
            seen["keep-alive sent alone"] += 1
    out["sync_count"] = 5 - st["remaining"]
    out["queue"] = max(0, i["newest"] - i["acked"])
    if shut:
        if len(out["msgs"]) + due[0] > 0:
            seen["the shutdown call zeroes that call's sends"] += 1
        out.update(input_length=0, ack_due=0, reply_due=0, report_due=0, keepalive_due=0, msgs=[])
        due[0] = 0
    sent = len(out["msgs"]) + due[0]
    st["sent"] += sent
    if sent > 0:
        st["last_send"] = now
    out["liveness"] = 1 if i["received"] or st["state"] != RUNNING else 0
    if st["state"] == SYNCING and not i["received"]:
        seen["liveness_received holds for a silent synchronizing endpoint"] += 1
    out["synchronized"] = 1 if st["state"] >= RUNNING else 0
    return out


def kbps_sent(st, now, message_bytes):
    """UdpProtocol::network_stats' kbps_sent, :279-301; None is NotSynchronized."""
    if st["state"] not in (SYNCING, RUNNING):
        return None
    seconds = (now - st["stats_start"]) // 1000
    if seconds == 0:
        return None
    return ((st["sent"] * message_bytes + st["sent"] * 28) // seconds) // 1024


# ---------------------------------------------------------------------------
# The schedule: a clock, and a scripted peer per endpoint
# ---------------------------------------------------------------------------
def clock():
    rng = np.random.default_rng(SEED)

    def pattern(total):
        while True:
            steps = rng.integers(11, 22, 12)
            steps[-1] = total - int(steps[:-1].sum())
            if 11 <= steps[-1] <= 21:
                return [int(x) for x in steps]
    p200, p201 = pattern(200), pattern(201)
    t = [EPOCH_MS]
    for c in range(1, CALLS):
        step = 300 if c == GAP_300 else 5000 + 37 if c == GAP_5000 else (p201 if GAP_300 < c < GAP_5000 else p200)[c % 12]
        t.append(t[-1] + step)
    return t


SCRIPTS = ["fast", "lossy", "silent", "dup", "pair", "tail", "flood", "disc_sync", "disc_run", "idle", "moved", "play"]


class Sched:
    pass


def moved_variant(h, s):
    return (s // len(SCRIPTS) + 5 * h) % 9


@functools.lru_cache(maxsize=None)
def schedule(P, sync_slots):
    """Every call's inputs, the state rows the caller writes before it, and what the model says the
    state and the outputs are after it, for all P x S endpoints; and the witness counter."""
    rng = np.random.default_rng(SEED + 100 * P + sync_slots)
    now = clock()
    sc = Sched()
    sc.P, sc.sync_slots, sc.now = P, sync_slots, now
    sc.magic = rng.integers(1, 65536, (P, S)).astype(np.uint16)
    peer = rng.integers(1, 65536, (P, S)).astype(np.uint16)
    peer[peer == sc.magic] ^= 0x55
    sc.seen = collections.Counter()
    sc.script = [[SCRIPTS[(s + 5 * h) % len(SCRIPTS)] for s in range(S)] for h in range(P)]
    # when the script begins: spread over the three parts of the clock
    begin = [[(2, GAP_300 + 2, 3, GAP_5000 + 2)[(s // len(SCRIPTS) + h) % 4] for s in range(S)] for h in range(P)]
    st = [[fresh() for _ in range(S)] for _ in range(P)]
    mem = [[{} for _ in range(S)] for _ in range(P)]
    resets = {60: [s for s in range(S) if s % 11 == 4], 100: [s for s in range(S) if s % 13 == 6]}
    sc.inputs, sc.loads, sc.outs, sc.states, sc.reports = [], [], [], [], []

    def newest_nonce(t, back=0):
        at = (t["next"] - 1 - back) & 7
        return t["nonces"][at] if (t["valid"] >> at) & 1 else None

    for c in range(CALLS):
        loads = []
        for s in resets.get(c, []):          # EndpointProtocol.reset: zeroed columns, and the script starts over
            for h in range(P):
                st[h][s] = fresh()
                mem[h][s] = {}
                begin[h][s] = c + 1 + (s + h) % 3
                loads.append((h, s, dict(st[h][s], nonces=[0] * 8)))
        reports = [int(rng.integers(0, 3)) if c % 7 == 3 and s % 3 == 0 else 0 for s in range(S)]
        for h in range(P):                   # a moved endpoint whose KeepAlive a ChecksumReport holds back
            for s in range(S):
                if sc.script[h][s] == "moved" and c == begin[h][s] and moved_variant(h, s) == 6:
                    reports[s] = max(reports[s], 1)
        ins = [[None] * S for _ in range(P)]
        outs = [[None] * S for _ in range(P)]
        for h in range(P):
            for s in range(S):
                t, m, kind, b = st[h][s], mem[h][s], sc.script[h][s], begin[h][s]
                pm, lm = int(peer[h, s]), int(sc.magic[h, s])
                i = {"call": c, "now": now[c], "magic": lm, "start": 0, "disconnected": 0, "ack_owed": 0, "reply_owed": 0,
                     "received": 0, "newest": NULL, "acked": NULL, "length": 0, "reports": reports[s], "slots": [],
                     "nonces": [int(x) for x in rng.integers(0, 2**32, M)]}
                slots = []
                k = c - b          # the script's own call count
                if kind == "moved" and k == 0:
                    # endpoints that arrive as state rows: the two 5000 ms boundaries, a KeepAlive due on its own
                    # and beside each other kind
                    v = moved_variant(h, s)
                    row = fresh()
                    if v < 2:
                        row.update(state=DISCONNECTED, shutdown_at=now[c] - v, remote_magic=pm)
                    else:
                        row.update(state=RUNNING, last_send=now[c] - 300, last_input_recv=now[c] - 20,
                                   last_quality_report=now[c] - 20, stats_start=now[c] - 300, remote_magic=pm, sent=9,
                                   last_newest=5)
                    m["v"] = v
                    st[h][s] = t = row
                    loads.append((h, s, dict(row, nonces=[0] * 8)))
                if kind == "moved" and k >= 0:
                    v = m["v"]
                    i.update(newest=4, acked=4, received=1)
                    if k == 0:
                        if v == 3:
                            i["ack_owed"] = 1
                        elif v == 4:
                            i["reply_owed"] = 1
                        elif v == 5:
                            i.update(newest=5, acked=3, length=9)
                        elif v == 7:
                            slots.append(m_sync_request(pm, 77))
                        elif v == 8:
                            t["last_quality_report"] = now[c] - 300
                            loads[-1][2]["last_quality_report"] = now[c] - 300
                    if v < 2 and k in (0, 1):
                        i["ack_owed"] = 1
                        slots.append(m_sync_request(pm, 5))
                elif kind != "moved":
                    if k == -1 and kind in ("fast", "tail"):
                        slots.append(m_sync_request(pm, 0x01020304))       # answered in Initializing
                    if k == 0:
                        i["start"] = 1
                        if kind == "flood":
                            slots += [m_sync_request(pm, 10 + j) for j in range(M)]
                    if kind == "dup":
                        i["nonces"] = [0xD0D0D0D0 + s] * M
                    running = t["state"] == RUNNING
                    if t["state"] == SYNCING and k > 0:
                        n0, n1 = newest_nonce(t), newest_nonce(t, 1)
                        if kind == "idle":
                            i.update(newest=3, length=11)                    # an input while synchronizing
                        if kind in ("fast", "flood", "disc_run", "play", "idle") or (kind == "dup" and t.get("retried")):
                            if n0 is not None:
                                slots.append(m_sync_reply(pm, n0))
                                if t["remaining"] == 1 and kind == "fast":   # the magic it sets drops the next slot
                                    slots.append(m_sync_request(pm ^ 0x0101, 9))
                        elif kind == "lossy":
                            i["newest"] = 3                                  # an input while synchronizing
                            i["length"] = 11
                            if k == 3:
                                slots.append((9, m_sync_reply(pm, n0)))        # truncated
                            if k == 5:
                                slots.append(m_sync_reply(pm, 0xBAD0BAD0))     # unknown
                            if t.get("retried") and n0 is not None:
                                slots.append(m_sync_reply(pm, n1 if n1 is not None else n0))
                        elif kind == "pair":                                 # both outstanding replies in one call
                            if t.get("retried") and n0 is not None and n1 is not None:
                                slots += [m_sync_reply(pm, n1), m_sync_reply(pm, n0)]
                            elif t.get("retried") and n0 is not None:
                                slots.append(m_sync_reply(pm, n0))
                        elif kind == "tail":                                 # the fifth good reply, then another
                            if t.get("retried"):
                                m.setdefault("spare", n1)
                                if t["remaining"] == 1:
                                    slots += [m_sync_reply(pm, n0), m_sync_reply(pm, m["spare"])]
                                elif n0 is not None:
                                    slots.append(m_sync_reply(pm, n0))
                        elif kind == "disc_sync" and k == 4:
                            i["disconnected"] = 4
                        elif kind == "silent" and bin(t["valid"]).count("1") == 8 and t.get("evicted"):
                            if not m.get("told"):
                                slots.append(m_sync_reply(pm, t["evicted"][0]))
                                m["told"] = True
                    if running:
                        r = m.setdefault("run", 0)
                        m["run"] += 1
                        i["received"] = 1
                        if kind in ("fast", "play", "disc_run", "dup", "pair", "tail", "flood"):
                            i["newest"] = r
                            i["acked"] = max(NULL, r - 3) if kind != "flood" else NULL + (r > 20) * (r - 5)
                            i["length"] = 7 + r % 5
                            i["ack_owed"] = 1 if r % 2 and kind != "tail" else 0
                            i["reply_owed"] = 1 if r % 13 == 5 else 0
                        if kind == "lossy":
                            i.update(newest=3, acked=NULL, length=11)     # held back while synchronizing
                        if kind == "idle":
                            i.update(newest=3, acked=NULL if r < 20 else 3, length=11, received=1 if r % 30 else 0)
                        if kind == "fast" and r == 3:
                            slots.append(m_sync_reply(pm, 123))              # a reply after Running
                            slots.append(m_sync_request(pm, 0xA0B0C0D0))     # answered in Running
                        if kind == "fast" and r == 6:
                            slots.append(m_sync_request(pm ^ 0x1000, 1))     # the magic filter
                        if kind == "disc_run" and r == 9:
                            i["disconnected"] = 1
                    if t["state"] == DISCONNECTED:
                        i["newest"] = m.get("run", 0) + 2
                        i["acked"] = NULL
                        if c % 3 == 0 or c == GAP_5000:
                            slots.append(m_sync_request(pm, c))              # answered in Disconnected
                            i["ack_owed"] = 1
                    if t["state"] == SHUTDOWN and c % 5 == 0:
                        slots.append(m_sync_request(pm, c))
                        i["ack_owed"] = 1
                i["slots"] = [(x if isinstance(x, tuple) else (len(x), x)) for x in slots[:M]]
                i["slots"] = [(n, bytes(d) + bytes(rng.integers(0, 256, STRIDE - len(d), dtype=np.uint8))) for n, d in i["slots"]]
                i["slots"] += [(0, bytes(STRIDE))] * (M - len(i["slots"]))
                ins[h][s] = i
                outs[h][s] = model_step(t, i, sync_slots, sc.seen)
                if i["received"] == 0 and t["state"] == SYNCING and c == GAP_5000:
                    sc.seen["synchronizing across a silent gap longer than the disconnect timeout"] += 1
        if P == 3:
            for s in range(S):
                states = sorted(st[h][s]["state"] for h in range(P))
                if states[0] == SYNCING and states[1] >= RUNNING:
                    sc.seen["session_running with one of three endpoints still synchronizing"] += 1
        sc.inputs.append(ins)
        sc.loads.append(loads)
        sc.outs.append(outs)
        sc.reports.append(reports)
        sc.states.append([[{k: (list(v) if isinstance(v, list) else v) for k, v in st[h][s].items()} for s in range(S)]
                          for h in range(P)])
    for s in {s for v in resets.values() for s in v}:
        if 0 < s < S - 1:
            sc.seen["a reset column beside untouched neighbours"] += 1
    sc.resets = resets
    return sc


STATE_ROW = ("state", "remaining", "valid", "next", "last_send", "last_input_recv", "last_quality_report", "shutdown_at",
             "stats_start", "sent", "last_newest", "remote_magic")


def state_line(t):
    return (f"{t['state']} {t['remaining']} " + " ".join(str(x) for x in t["nonces"]) + f" {t['valid']} {t['next']} {t['last_send']} "
            f"{t['last_input_recv']} {t['last_quality_report']} {t['shutdown_at']} {t['stats_start']} {t['sent']} {t['last_newest']} "
            f"{t['remote_magic']}")


def out_line(o, sync_slots):
    msgs = [m.hex() for m in o["msgs"]] + ["-"] * (sync_slots - len(o["msgs"]))
    return (f"{o['input_length']} {o['ack_due']} {o['reply_due']} {o['report_due']} {o['keepalive_due']} {len(o['msgs'])} {o['events']} "
            f"{o['sync_count']} {o['liveness']} {o['queue']} {o['synchronized']} {o['status']} | " + " ".join(msgs))


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point():
    header = open(os.path.join(ROOT, "include", "ggrs_amd.h")).read()
    lib = L.load()
    name = "rb_endpoint_protocol_poll_all"
    assert f"rb_status {name}(" in header and hasattr(lib, name) and name in [n for n, _, _ in L.SIGNATURES]
    for k, v in [("RB_EP_INITIALIZING", 0), ("RB_EP_SYNCHRONIZING", 1), ("RB_EP_RUNNING", 2), ("RB_EP_DISCONNECTED", 3),
                 ("RB_EP_SHUTDOWN", 4)]:
        assert f"#define {k} {v}" in header and getattr(L, k) == v
    for cited in (":325-333", ":335-341", ":351-404", ":429-432", ":444-446", ":527-538", ":546-548", ":578-583", ":586-614",
                  ":372-375", ":279-301"):
        assert cited in header, cited
    # the struct as ctypes lays it out is the header's: pointers, int64 and one int32 pair
    body = header.split("typedef struct rb_endpoint_protocol {")[1].split("} rb_endpoint_protocol;")[0]
    fields = [ln.strip().rstrip(";").split()[-1].lstrip("*") for ln in body.splitlines() if ln.strip().endswith(";")]
    assert fields == [f for f, _ in L.RbEndpointProtocol._fields_]
    assert ctypes.sizeof(L.RbEndpointProtocol) == 8 * (len(fields) - 1)
    assert "RB_PLUGIN_ABI 8" in open(os.path.join(ROOT, "include", "ggrs_amd_game.hpp")).read()
    assert callable(G.EndpointProtocol)


def test_known_answer_sync_datagrams():
    assert m_sync_request(0x1234, 0x12345678) == bytes.fromhex("34120000000078563412")
    assert m_sync_reply(0x1234, 0x12345678) == bytes.fromhex("34120100000078563412")
    st = fresh()
    i = {"call": 0, "now": 1000, "magic": 0x1234, "start": 1, "disconnected": 0, "ack_owed": 0, "reply_owed": 0, "received": 0,
         "newest": NULL, "acked": NULL, "length": 0, "reports": 0, "slots": [(10, m_sync_request(0x4321, 7))],
         "nonces": [0x12345678, 2, 3, 4]}
    o = model_step(st, i, 4)
    assert o["msgs"] == [bytes.fromhex("34120000000078563412"), m_sync_reply(0x1234, 7)]
    assert (st["state"], st["remaining"], st["sent"], st["last_send"], st["valid"], st["next"]) == (SYNCING, 5, 2, 1000, 1, 1)


def test_the_kbps_formula():
    st = dict(fresh(), state=RUNNING, stats_start=10_000, sent=700)
    assert kbps_sent(st, 10_999, 56) is None                       # seconds == 0
    assert kbps_sent(st, 12_500, 56) == (700 * (56 + 28) // 2) // 1024 == 28
    assert kbps_sent(dict(st, state=SYNCING), 12_500, 56) == 28
    for state in (INIT, DISCONNECTED, SHUTDOWN):
        assert kbps_sent(dict(st, state=state), 12_500, 56) is None


_PROGRAMS = {}


def check_program(tmp_path_factory, sanitize=False):
    if sanitize in _PROGRAMS:
        return _PROGRAMS[sanitize]
    exe = _PROGRAMS[sanitize] = str(tmp_path_factory.mktemp("check_protocol") / "check_protocol")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O1"]
    subprocess.run(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-I", _CSRC, "-o", exe,
                    os.path.join(_TESTS, "check_protocol.cpp")], check=True)
    return exe


def schedule_file(sc, path, calls=CALLS):
    P = sc.P
    lines = [f"{P} {P * S} {M} {sc.sync_slots} {STRIDE} {calls}"]
    for c in range(calls):
        lines.append(f"{sc.now[c]} {len(sc.loads[c])}")
        lines += [f"{h * S + s} {state_line(row)}" for h, s, row in sc.loads[c]]
        for h in range(P):
            for s in range(S):
                i = sc.inputs[c][h][s]
                lines.append(f"{i['magic']} {i['start']} {i['disconnected']} {i['ack_owed']} {i['reply_owed']} {i['received']} "
                             f"{i['newest']} {i['acked']} {i['length']} {i['reports']} | "
                             + " ".join(f"{n} {d[:min(n, STRIDE)].hex() if n > 0 else '-'}" for n, d in i["slots"])
                             + " | " + " ".join(str(x) for x in i["nonces"]))
    path.write_text("\n".join(lines) + "\n")


def model_lines(sc, calls=CALLS):
    return [f"{c} {h * S + s} {state_line(sc.states[c][h][s])} | {out_line(sc.outs[c][h][s], sc.sync_slots)}"
            for c in range(calls) for h in range(sc.P) for s in range(S)]


@pytest.mark.parametrize("P,sync_slots", GEOMS)
def test_the_step_on_the_host_equals_the_model(tmp_path, tmp_path_factory, P, sync_slots):
    """tests/check_protocol.cpp drives protocol_step.hpp, the function the kernel calls, over every
    endpoint and call of the schedule, each datagram in a heap buffer of exactly its bytes."""
    sc = schedule(P, sync_slots)
    path = tmp_path / "schedule.txt"
    schedule_file(sc, path)
    r = subprocess.run([check_program(tmp_path_factory), "run", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    got, want = r.stdout.splitlines(), model_lines(sc)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


def test_the_step_under_the_sanitizers_on_the_schedule_and_on_corrupt_rows(tmp_path, tmp_path_factory):
    """The same stand-alone program built with -fsanitize=address,undefined: the schedule at P = 3,
    and state rows and inputs of random bytes (corrupt ep_state, sync_next, sync_valid, stamps)."""
    sc = schedule(3, 2)
    path = tmp_path / "schedule.txt"
    schedule_file(sc, path)
    exe = check_program(tmp_path_factory, True)
    r = subprocess.run([exe, "run", str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.splitlines() == model_lines(sc)
    r = subprocess.run([exe, "corrupt", "7", "200000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("corrupt ok 200000"), r.stdout + r.stderr[-3000:]


WITNESS = [
    "handshake finished in five round trips", "handshake finished after a retry",
    "a reply with an unknown nonce", "a reply to an evicted nonce", "a duplicate nonce from the caller", "a reply after Running",
    "two good replies in one call", "the fifth good reply followed by another in the same call",
    f"request answered in state {INIT}", f"request answered in state {RUNNING}", f"request answered in state {DISCONNECTED}",
    "request unanswered in Shutdown", "magic filter drops a sync message",
    "magic filter with the magic an earlier slot of the call set", "a truncated 9-byte sync datagram",
    "more sync messages than sync_slots", "resend with pending output", "resend with none: the stamp resets, no Input",
    "keep-alive sent alone", f"a new input in state {SYNCING} is not sent", "an input held back is not sent late once Running",
    "an input of the Synchronizing time leaves by the resend timer",
    f"disconnected in state {SYNCING}", f"disconnected in state {RUNNING}", "the shutdown call zeroes that call's sends",
    "liveness_received holds for a silent synchronizing endpoint",
    "synchronizing across a silent gap longer than the disconnect timeout", "a reset column beside untouched neighbours",
] + [f"keep-alive suppressed by {k} alone" for k in ("sync message", "InputAck", "QualityReply", "QualityReport", "Input",
                                                      "ChecksumReport")] \
  + [f"{t}: {b}" for t in ("sync retry", "resend", "quality report", "keep-alive", "shutdown")
     for b in ("now == stamp + delay, nothing fires", "now == stamp + delay + 1 fires")]


@pytest.mark.parametrize("P,sync_slots", GEOMS)
def test_the_schedule_shows_every_situation(P, sync_slots):
    """Counted on the model alone."""
    sc = schedule(P, sync_slots)
    missing = [w for w in WITNESS if sc.seen[w] == 0]
    assert not missing, missing
    if P == 3:
        assert sc.seen["session_running with one of three endpoints still synchronizing"] > 0
    now = sc.now
    steps = [b - a for a, b in zip(now, now[1:])]
    assert sorted(x for x in steps if not 11 <= x <= 21) == [300, 5037]
    # packets_sent, send_queue_len and kbps_sent take more than one value, seconds == 0 among them
    last, first = sc.states[-1], sc.states[5]
    assert len({t["sent"] for row in last for t in row}) > 10
    assert len({o["queue"] for call in sc.outs for row in call for o in row}) > 3
    assert any(kbps_sent(t, now[5], 56) is None and t["state"] == SYNCING for row in first for t in row)
    assert any((kbps_sent(t, now[-1], 56) or 0) > 0 for row in last for t in row)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
GUARD = 256
SENT = 0xA5
STATE_NAMES = ("ep_state", "sync_remaining", "sync_nonces", "sync_valid", "sync_next", "stamps", "packets_sent", "last_newest",
               "remote_magic")
OUT_NAMES = ("input_lengths", "ack_due", "reply_due", "report_due", "keepalive_due", "sync_lengths", "sync_counts", "events_mask",
             "sync_count", "liveness_received", "send_queue_len", "session_running", "status")


def guarded(shape, dtype, fill=None):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    pad = (-n) % 16
    buf = torch.full((GUARD + n + pad + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    view = buf[GUARD:GUARD + n].view(dtype).view(shape)
    if fill is not None:
        view.fill_(fill)
    return buf, view, n


class GuardedProtocol:
    """An EndpointProtocol whose every tensor sits between guards: the state rows of the handles
    served start zero (fresh), everything else is prefilled with SENT bytes."""

    def __init__(self, P, sync_slots, served):
        self.ep = G.EndpointProtocol(P, S, "cuda", sync_slots)
        self.ep.sync_datagrams = torch.zeros((sync_slots, P, S, STRIDE), dtype=torch.uint8, device="cuda")
        self.bufs = {}
        for name in STATE_NAMES + OUT_NAMES + ("sync_datagrams",):
            t = getattr(self.ep, name)
            buf, view, n = guarded(tuple(t.shape), t.dtype)
            if name in STATE_NAMES:
                view[..., served, :] = 0
            self.bufs[name] = (buf, n)
            setattr(self.ep, name, view)

    def host(self):
        return {name: getattr(self.ep, name).cpu().numpy() for name in self.bufs}

    def intact(self):
        for buf, n in self.bufs.values():
            b = buf.cpu().numpy()
            if not ((b[:GUARD] == SENT).all() and (b[GUARD + n:] == SENT).all()):
                return False
        return True


def write_row(ep, h, s, row):
    """The caller's way in: a state row written as load_state_dict writes a column."""
    ep.ep_state[h, s] = row["state"]
    ep.sync_remaining[h, s] = row["remaining"]
    ep.sync_nonces[:, h, s] = torch.tensor(np.array(row["nonces"], np.uint32).view(np.int32), device="cuda")
    ep.sync_valid[h, s] = row["valid"]
    ep.sync_next[h, s] = row["next"]
    ep.stamps[:, h, s] = torch.tensor([row[k] for k in STATE_ROW[4:9]], dtype=torch.int64, device="cuda")
    ep.packets_sent[h, s] = row["sent"]
    ep.last_newest[h, s] = row["last_newest"]
    ep.remote_magic[h, s] = int(np.array(row["remote_magic"], np.uint16).view(np.int16))


def call_tensors(sc, c):
    P = sc.P
    a = {k: np.zeros((P, S), np.uint8) for k in ("start", "disconnected", "ack_owed", "reply_owed", "received")}
    b = {k: np.zeros((P, S), np.int32) for k in ("newest", "acked", "length")}
    dg = np.zeros((M, P, S, STRIDE), np.uint8)
    ln = np.zeros((M, P, S), np.int32)
    nonces = np.zeros((M, P, S), np.uint32)
    for h in range(P):
        for s in range(S):
            i = sc.inputs[c][h][s]
            for k in a:
                a[k][h, s] = i[k]
            for k in b:
                b[k][h, s] = i[k]
            nonces[:, h, s] = i["nonces"]
            for m, (n, d) in enumerate(i["slots"]):
                dg[m, h, s] = np.frombuffer(d, np.uint8)
                ln[m, h, s] = n
    reports = np.zeros((K, S, 3), np.int64)
    reports[:, :, 2] = -1
    for s in range(S):
        # a session's own reports: the inputs carry them per endpoint because one script may add one
        n = max(sc.inputs[c][h][s]["reports"] for h in range(P))
        reports[:n, s, 2] = (c + np.arange(n)) | (-1 << 32)
    t = {k: torch.from_numpy(v).cuda() for k, v in {**a, **b}.items()}
    t.update(dg=torch.from_numpy(dg).cuda(), ln=torch.from_numpy(ln).cuda(),
             nonces=torch.from_numpy(nonces.view(np.int32)).cuda(), reports=torch.from_numpy(reports).cuda())
    return t


def expect_arrays(sc, c, hs):
    """The model's state and outputs after call c as arrays in the tensors' layout, for handles hs."""
    P, Q = sc.P, sc.sync_slots
    e = {"ep_state": np.zeros((P, S), np.uint8), "sync_remaining": np.zeros((P, S), np.int32),
         "sync_nonces": np.zeros((8, P, S), np.uint32), "sync_valid": np.zeros((P, S), np.uint8),
         "sync_next": np.zeros((P, S), np.uint8), "stamps": np.zeros((5, P, S), np.int64),
         "packets_sent": np.zeros((P, S), np.int64), "last_newest": np.zeros((P, S), np.int32),
         "remote_magic": np.zeros((P, S), np.uint16), "input_lengths": np.zeros((P, S), np.int32),
         "ack_due": np.zeros((P, S), np.uint8), "reply_due": np.zeros((P, S), np.uint8), "report_due": np.zeros((P, S), np.uint8),
         "keepalive_due": np.zeros((P, S), np.uint8), "sync_lengths": np.zeros((Q, P, S), np.int32),
         "sync_counts": np.zeros((P, S), np.int32), "events_mask": np.zeros((P, S), np.uint8),
         "sync_count": np.zeros((P, S), np.int32), "liveness_received": np.zeros((P, S), np.uint8),
         "send_queue_len": np.zeros((P, S), np.int32), "status": np.zeros((P, S), np.int32),
         "session_running": np.ones((S,), np.uint8)}
    for h in hs:
        for s in range(S):
            t, o = sc.states[c][h][s], sc.outs[c][h][s]
            e["ep_state"][h, s], e["sync_remaining"][h, s] = t["state"], t["remaining"]
            e["sync_nonces"][:, h, s] = t["nonces"]
            e["sync_valid"][h, s], e["sync_next"][h, s] = t["valid"], t["next"]
            e["stamps"][:, h, s] = [t[k] for k in STATE_ROW[4:9]]
            e["packets_sent"][h, s], e["last_newest"][h, s], e["remote_magic"][h, s] = t["sent"], t["last_newest"], t["remote_magic"]
            e["input_lengths"][h, s] = o["input_length"]
            for k in ("ack_due", "reply_due", "report_due", "keepalive_due", "sync_count", "status"):
                e[k][h, s] = o[k]
            e["sync_lengths"][:len(o["msgs"]), h, s] = 10
            e["sync_counts"][h, s] = len(o["msgs"])
            e["events_mask"][h, s], e["liveness_received"][h, s], e["send_queue_len"][h, s] = o["events"], o["liveness"], o["queue"]
            e["session_running"][s] &= o["synchronized"]
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("P,sync_slots,mask", CASES)
def test_gpu_kernel_equals_the_model_inside_guards(gpu_available, P, sync_slots, mask):
    """After every call of the schedule every state row and every output of every endpoint served
    equals the model's, the sync datagrams byte for byte; rows of other handles keep their prefill,
    the inputs are unchanged and the guards stay."""
    sc = schedule(P, sync_slots)
    hs = handles_of(mask, P)
    others = [h for h in range(P) if h not in hs]
    gp = GuardedProtocol(P, sync_slots, hs)
    ep = gp.ep
    magic = torch.from_numpy(sc.magic.view(np.int16)).cuda()
    before = gp.host()
    want_dg = np.full((sync_slots, P, S, STRIDE), SENT, np.uint8)
    for c in range(CALLS):
        for h, s, row in sc.loads[c]:
            if h in hs:
                write_row(ep, h, s, row)
        t = call_tensors(sc, c)
        keep = {k: v.clone() for k, v in t.items()}
        ep.poll(mask, sc.now[c], magic, t["dg"], t["ln"], nonces=t["nonces"], start=t["start"], disconnected=t["disconnected"],
                ack_owed=t["ack_owed"], reply_owed=t["reply_owed"], received=t["received"], newest=t["newest"], acked=t["acked"],
                lengths=t["length"], reports=t["reports"])
        got = gp.host()
        want = expect_arrays(sc, c, hs)
        for k, v in keep.items():
            assert torch.equal(t[k], v), f"input {k}, call {c}"
        for name, w in want.items():
            g = got[name]
            if name == "session_running":
                assert np.array_equal(g, w), f"{name}, call {c}"
                continue
            g = g.view(w.dtype) if g.dtype != w.dtype else g
            bad = np.argwhere(g[..., hs, :] != w[..., hs, :])
            assert bad.size == 0, f"{name}, call {c}: first at {bad[0]}: {g[..., hs, :][tuple(bad[0])]} != {w[..., hs, :][tuple(bad[0])]}"
            assert np.array_equal(got[name][..., others, :], before[name][..., others, :]), f"{name}: rows outside the mask, call {c}"
        for h in hs:
            for s in range(S):
                for m, data in enumerate(sc.outs[c][h][s]["msgs"]):
                    want_dg[m, h, s, :16] = np.frombuffer(data + bytes(6), np.uint8)
        assert np.array_equal(got["sync_datagrams"], want_dg), f"sync datagrams, call {c}"
        assert gp.intact(), f"guards, call {c}"


@pytest.mark.gpu
def test_gpu_invalid_requests_leave_every_tensor_as_it_was(gpu_available):
    P, Q = 3, 2
    sc = schedule(P, Q)
    gp = GuardedProtocol(P, Q, [0, 1, 2])
    ep = gp.ep
    magic = torch.from_numpy(sc.magic.view(np.int16)).cuda()
    t = call_tensors(sc, 2)
    before = gp.host()
    lib = L.load()

    def request(mask=0b111, players=P, **change):
        io = L.RbEndpointProtocol(
            **{k: ctypes.c_void_p(getattr(ep, k).data_ptr()) for k in STATE_NAMES},
            now_ms=sc.now[2], local_magic=magic.data_ptr(), start=t["start"].data_ptr(), datagrams=t["dg"].data_ptr(),
            stride=STRIDE, slots=M, sync_slots=Q, dg_lengths=t["ln"].data_ptr(), nonces=t["nonces"].data_ptr(),
            disconnected=None, ack_owed=None, reply_owed=None, received=None, newest=t["newest"].data_ptr(),
            acked=t["acked"].data_ptr(), lengths=None, reports=None, input_lengths=ep.input_lengths.data_ptr(),
            ack_due=ep.ack_due.data_ptr(), reply_due=ep.reply_due.data_ptr(), report_due=ep.report_due.data_ptr(),
            keepalive_due=ep.keepalive_due.data_ptr(), sync_datagrams=ep.sync_datagrams.data_ptr(),
            sync_lengths=ep.sync_lengths.data_ptr(), sync_counts=ep.sync_counts.data_ptr(), events=ep.events_mask.data_ptr(),
            sync_count=ep.sync_count.data_ptr(), liveness_received=None, send_queue_len=None, session_running=None,
            status=ep.status.data_ptr())
        for k, v in change.items():
            setattr(io, k, v)
        stream = torch.cuda.current_stream().cuda_stream
        return lib.rb_endpoint_protocol_poll_all(0, ctypes.c_void_p(stream), mask, players, S, ctypes.byref(io))

    refused = [dict(mask=0), dict(mask=0b1000), dict(players=5, mask=0b1), dict(slots=0), dict(slots=9), dict(sync_slots=0),
               dict(sync_slots=9), dict(stride=0), dict(stride=24), dict(stride=8), dict(now_ms=-1),
               dict(datagrams=t["dg"].data_ptr() + 8), dict(sync_datagrams=ep.sync_datagrams.data_ptr() + 4)]
    refused += [{k: None} for k in STATE_NAMES] + [{k: None} for k in (
        "local_magic", "datagrams", "dg_lengths", "nonces", "newest", "acked", "input_lengths", "ack_due", "reply_due", "report_due",
        "keepalive_due", "sync_datagrams", "sync_lengths", "sync_counts", "events", "sync_count", "status")]
    for change in refused:
        assert request(**change) == L.RB_INVALID_REQUEST, change
    torch.cuda.synchronize()
    after = gp.host()
    for name in before:
        assert np.array_equal(before[name], after[name]), name
    assert gp.intact()
    # and the request itself, with every optional tensor NULL, is served
    assert request() == L.RB_OK
    torch.cuda.synchronize()
    assert gp.intact() and (gp.host()["ep_state"] == np.array([[sc.states[2][h][s]["state"] if sc.inputs[2][h][s]["start"] else 0
                                                                 for s in range(S)] for h in range(P)], np.uint8)).all()


# ---------------------------------------------------------------------------
# GPU: two batches that know only each other's address
# ---------------------------------------------------------------------------
LINK_CALLS = 238
LINK_LATE, LINK_RESET, LINK_STOP, LINK_END_GAP = 40, 120, 200, 230
LINK_Q, LINK_B = 4, 4          # sync slots and build slots a side sends per call: 8 incoming slots


def link_clock():
    t, out = EPOCH_MS, []
    for c in range(LINK_CALLS):
        # silent for longer than the disconnect timeout (2000 ms) early on; 100 ms a call once the links are cut
        t += 2500 if c == 3 else 5100 if c == LINK_END_GAP else 100 if c > LINK_STOP else 16
        out.append(t)
    return out


class LinkSide:
    def __init__(self, local, magic, X, rng):
        from test_time_sync import make_session
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        self.local, self.remote = local, 1 - local
        self.mask = 1 << self.remote                       # the endpoint row is the remote handle's
        self.ep = G.EndpointProtocol(2, S, "cuda", LINK_Q)
        self.parsed = G.ParsedDatagrams(2, S, 64)
        self.sess = make_session(G.Game.EX_GAME, 2, 1 << local, 0, 0, sessions=S, time_sync=False)
        self.sess.enable_liveness()
        self.magic = torch.from_numpy(magic.view(np.int16)).cuda()
        self.m_magic = magic
        self.state_out = z((2, S), torch.uint8)
        self.disc = z((2, S), torch.uint8)
        self.out_dg, self.out_ln = z((LINK_B, 2, S, STRIDE), torch.uint8), z((LINK_B, 2, S), torch.int32)
        self.out_cnt, self.out_st = z((2, S), torch.int32), z((2, S), torch.int32)
        self.nulls = torch.full((2, S), NULL, dtype=torch.int32, device="cuda")
        self.zeros8, self.zeros32 = z((2, S), torch.uint8), z((2, S), torch.int32)
        self.sent_dg = z((LINK_Q + LINK_B, 2, S, STRIDE), torch.uint8)     # what left last call
        self.sent_ln = z((LINK_Q + LINK_B, 2, S), torch.int32)
        self.frame = np.zeros(S, np.int64)                  # ticks run per session, on the host
        self.m_state = [fresh() for _ in range(S)]
        self.X, self.dX = X, torch.from_numpy(X).cuda()
        self.rng = rng


@pytest.mark.gpu
def test_gpu_two_batches_connect_over_datagrams_and_gate_their_ticks(gpu_available):
    """Two ex_game batches (P = 2, S = 70), each local to one handle, with random distinct magics and
    remote_magic 0, exchange nothing but datagrams: parse -> protocol -> liveness -> paced tick ->
    build -> gate, the sync datagrams concatenated to build's along the slot axis, a tenth of all
    datagrams lost.  Every third pair starts 40 calls late; the clock is silent for 2500 ms (the
    disconnect timeout is 2000 ms) while everyone still synchronizes; every fifth pair is reset at call
    120; the link of every seventh pair is cut at call 200, and after 5100 ms more its endpoints are
    in Shutdown.  After every call the endpoint state, the outputs and every sync datagram byte equal
    the model's (fed what parse and liveness returned), session_running is the run mask, and the
    batch's frames are the ticks the model let it run.  The Inputs themselves do not travel as
    datagrams here: each batch reads its peer's inputs from the truth tensor."""
    now = link_clock()
    rng = np.random.default_rng(0x20C0)
    magics = rng.permutation(np.arange(1, 65536))[:2 * S].astype(np.uint16).reshape(2, S)     # distinct
    F = LINK_CALLS + 1
    X = G.synth_inputs(S, 2, F, seed=G.SEED ^ 0x20)
    stream = torch.cuda.Stream()
    late = np.arange(S) % 3 == 2
    fifth, cut = np.arange(S) % 5 == 4, np.arange(S) % 7 == 3
    with torch.cuda.stream(stream):
        sides = [LinkSide(i, np.ascontiguousarray(np.broadcast_to(magics[i], (2, S))), X, rng) for i in (0, 1)]
        for side in sides:
            side.sess.set_stream(stream)
        parked = timed_out_early = 0
        for c in range(LINK_CALLS):
            lost = rng.random((2, LINK_Q + LINK_B, 2, S)) < 0.1
            if c >= LINK_STOP:
                lost[:, :, :, cut] = True
            start = np.zeros((2, S), np.uint8)
            start[:, (~late if c == 0 else late if c == LINK_LATE else fifth if c == LINK_RESET + 1 else np.zeros(S, bool))] = 1
            if c == LINK_RESET:
                for side in sides:
                    side.ep.reset(torch.from_numpy(np.flatnonzero(fifth)).cuda())
                    side.sess.restart_sessions(fifth)
                    side.parsed.acked[:, fifth] = NULL
                    side.frame[fifth] = 0
                    side.disc[:, fifth] = 0
                    for s in np.flatnonzero(fifth):
                        side.m_state[s] = fresh()
            heard = []
            for i, side in enumerate(sides):     # what the peer sent last call, in this side's row, minus the lost
                peer = sides[1 - i]
                dg = peer.sent_dg.flip(1).contiguous()
                ln = (peer.sent_ln.flip(1) * torch.from_numpy((~lost[i]).astype(np.int32)).cuda()).contiguous()
                heard.append((dg, ln))
            for i, side in enumerate(sides):
                ep, r = side.ep, side.remote
                dg, ln = heard[i]
                nonces = rng.integers(0, 2**32, (LINK_Q + LINK_B, 2, S), dtype=np.uint32)
                G.parse_datagrams(side.parsed, side.mask, dg, ln, ep.remote_magic, now[c])
                ep.poll(side.mask, now[c], side.magic, dg, ln, nonces=torch.from_numpy(nonces.view(np.int32)).cuda(),
                        start=torch.from_numpy(start).cuda(), disconnected=side.disc, reply_owed=side.parsed.reply_owed,
                        received=side.parsed.received)
                side.sess.poll_liveness(now[c], ep.liveness_received, state_out=side.state_out)
                run = ep.session_running.cpu().numpy()
                li = torch.from_numpy(X[side.frame, :, np.arange(S)].T.copy()[None]).cuda()       # [1, P, S]
                upto = torch.from_numpy(np.broadcast_to(side.frame.astype(np.int32), (1, 2, S)).copy()).cuda()
                side.sess.run_ticks(li, upto, side.dX, run_mask=ep.session_running[None].contiguous())
                G.build_datagrams(side.mask, side.out_dg, side.out_ln, side.out_cnt, side.out_st, side.magic, now[c], side.nulls,
                                  side.nulls, side.zeros8, reply_owed=ep.reply_due, reply_ping=side.parsed.reply_ping,
                                  report_due=ep.report_due, frame_advantage=side.zeros32, keepalive_due=ep.keepalive_due)
                ep.gate(side.out_ln, side.out_cnt)
                # the model, fed the same datagrams and what parse and liveness returned
                h_dg, h_ln = dg.cpu().numpy(), ln.cpu().numpy()
                h_recv, h_owed = side.parsed.received.cpu().numpy(), side.parsed.reply_owed.cpu().numpy()
                h_disc = side.disc.cpu().numpy()
                got = {k: getattr(ep, k).cpu().numpy() for k in STATE_NAMES + OUT_NAMES + ("sync_datagrams",)}
                events = ep.events()
                for s in range(S):
                    st = side.m_state[s]
                    inp = {"call": c, "now": now[c], "magic": int(side.m_magic[r, s]), "start": int(start[r, s]),
                           "disconnected": int(h_disc[r, s]), "ack_owed": 0, "reply_owed": int(h_owed[r, s]),
                           "received": int(h_recv[r, s]), "newest": NULL, "acked": NULL, "length": 0, "reports": 0,
                           "slots": [(int(h_ln[m, r, s]), h_dg[m, r, s].tobytes()) for m in range(LINK_Q + LINK_B)],
                           "nonces": [int(x) for x in nonces[:, r, s]]}
                    o = model_step(st, inp, LINK_Q)
                    what = f"call {c}, side {i}, session {s}"
                    assert (got["ep_state"][r, s], got["sync_remaining"][r, s], got["sync_valid"][r, s], got["sync_next"][r, s],
                            got["packets_sent"][r, s], got["last_newest"][r, s], int(got["remote_magic"].view(np.uint16)[r, s])) == \
                        (st["state"], st["remaining"], st["valid"], st["next"], st["sent"], st["last_newest"], st["remote_magic"]), what
                    assert got["sync_nonces"].view(np.uint32)[:, r, s].tolist() == st["nonces"], what
                    assert got["stamps"][:, r, s].tolist() == [st[k] for k in STATE_ROW[4:9]], what
                    assert (got["input_lengths"][r, s], got["ack_due"][r, s], got["reply_due"][r, s], got["report_due"][r, s],
                            got["keepalive_due"][r, s], got["sync_counts"][r, s], got["events_mask"][r, s], got["sync_count"][r, s],
                            got["liveness_received"][r, s], got["send_queue_len"][r, s], got["status"][r, s], run[s]) == \
                        (0, 0, o["reply_due"], o["report_due"], o["keepalive_due"], len(o["msgs"]), o["events"], o["sync_count"],
                         o["liveness"], 0, o["status"], o["synchronized"]), what
                    for m, data in enumerate(o["msgs"]):
                        assert got["sync_datagrams"][m, r, s, :16].tobytes() == data + bytes(6), what
                    assert got["sync_lengths"][:, r, s].tolist() == [10] * len(o["msgs"]) + [0] * (LINK_Q - len(o["msgs"])), what
                    want_ev = ([("Synchronizing", r, 5, o["sync_count"])] if o["events"] & EV_SYNCHRONIZING else []) + \
                        ([("Synchronized", r)] if o["events"] & EV_SYNCHRONIZED else [])
                    assert events[s] == want_ev, what
                    if st["state"] >= SHUTDOWN:
                        assert not side.out_ln[:, r, s].any() and side.out_cnt[r, s] == 0, f"gate, {what}"
                    if o["synchronized"]:
                        side.frame[s] += 1
                    parked += int(not o["synchronized"])
                # a session advances exactly when the model lets it, until liveness disconnects its peer: the
                # batch's own handling of that disconnect (tests/test_liveness.py) is followed from then on
                cur = side.sess.frames()[0]
                gone = (side.sess.read_liveness()[1][r] & 4) != 0
                side.frame[gone] = cur[gone]
                assert np.array_equal(cur, side.frame), (f"frames, call {c}, side {i}: sessions {np.flatnonzero(cur != side.frame)} at "
                                                         f"{cur[cur != side.frame]}, the model at {side.frame[cur != side.frame]}; liveness "
                                                         f"{side.sess.read_liveness()[1][:, cur != side.frame]}, events "
                                                         f"{side.sess.network_events()[1][cur != side.frame]}, peer state "
                                                         f"{[sides[1 - i].m_state[s]['state'] for s in np.flatnonzero(cur != side.frame)]}")
                side.disc = ((side.state_out & 4) != 0).to(torch.uint8)
                side.sent_dg = torch.cat([ep.sync_datagrams, side.out_dg])
                side.sent_ln = torch.cat([ep.sync_lengths, side.out_ln])
                if c < LINK_STOP:      # nobody is timed out, synchronizing or running, across the silent gap included
                    timed_out_early += int(gone.sum())
            states = np.array([[st["state"] for st in side.m_state] for side in sides])
            if c == 2:
                assert (states[:, ~late] == SYNCING).all() and (states[:, late] == INIT).all()
            if c == LINK_LATE - 1:
                assert (states[:, late] == INIT).all() and (states[:, ~late] == RUNNING).any()
            if c == LINK_RESET - 1 or c == LINK_STOP - 1:
                assert (states >= SYNCING).all() and (states == RUNNING).mean() > 0.5, f"call {c}"
                for i, side in enumerate(sides):     # whoever finished learned its peer's magic
                    assert all(st["remote_magic"] == (int(magics[1 - i][s]) if st["state"] == RUNNING else 0)
                               for s, st in enumerate(side.m_state))
                was_running = states == RUNNING
            if c == LINK_RESET:
                assert (states[:, fifth] == INIT).all() and (states[:, ~fifth] >= SYNCING).all()
            if c == LINK_STOP - 1:   # the reset pairs play from frame 0 while their neighbours played on
                for j, side in enumerate(sides):
                    again = fifth & was_running[j]
                    assert again.any() and (side.frame[again] > 0).all() and (side.frame[again] < LINK_STOP - LINK_RESET).all()
                    assert (side.frame[~fifth & ~late & was_running[j]] > LINK_STOP - LINK_RESET).any()
            if c == LINK_END_GAP - 1:   # liveness disconnected the endpoints whose peer went silent, and only those
                assert (states[:, cut][was_running[:, cut]] == DISCONNECTED).all() and was_running[:, cut].any()
                assert (states[:, ~cut] == was_running[:, ~cut] * RUNNING + ~was_running[:, ~cut] * states[:, ~cut]).all()
            if c >= LINK_END_GAP:
                assert (states[:, cut][was_running[:, cut]] == SHUTDOWN).all()
        assert parked >= 2 * 40 * int(late.sum()) and timed_out_early == 0
        # the send half of NetworkStats against the formula, and a session's endpoints travelling by plain indexing
        for side in sides:
            stats = side.ep.network_stats(now[-1], 56)
            want = [kbps_sent(st, now[-1], 56) for st in side.m_state]
            assert stats["kbps_sent"][side.remote].tolist() == [-1 if k is None else k for k in want]
            assert not stats["send_queue_len"][side.remote].any()
            idx = torch.tensor([1, 5, 9], device="cuda")
            kept = side.ep.state_dict(idx)
            whole = {k: v.clone() for k, v in side.ep.state_dict().items()}
            side.ep.reset(idx)
            assert all(not v[..., idx].any() for v in side.ep.state_dict().values())
            assert all(torch.equal(v[..., 2], whole[k][..., 2]) for k, v in side.ep.state_dict().items())
            side.ep.load_state_dict(kept, idx)
            assert all(torch.equal(v, whole[k]) for k, v in side.ep.state_dict().items())
            side.sess.close()


# ---------------------------------------------------------------------------
# GPU: the whole frame loop.  Two batches shake hands, then play each other over datagrams only
# ---------------------------------------------------------------------------
LOBBY_CAP = 1200      # calls the handshake of every pair may take at most (see DESIGN.md section 20 on held-off retries)
PLAY_CALLS = 60


class Endpoints:
    """One side's EndpointProtocol (row h: the endpoint that sends local handle h's inputs and hears the
    peer's row partner[h]) with the model's rows beside it."""

    def __init__(self, P, mask, n, magic):
        self.P, self.mask, self.n = P, mask, n
        self.hs = handles_of(mask, P)
        self.pt = [(h + P // 2) % P for h in range(P)]
        self.ep = G.EndpointProtocol(P, n, "cuda", LINK_Q)
        self.magic = torch.full((P, n), magic, dtype=torch.int16, device="cuda")
        self.m_magic = magic
        self.m_state = [[fresh() for _ in range(n)] for _ in range(P)]
        self.sent_dg = torch.zeros((LINK_Q + LINK_B, P, n, STRIDE), dtype=torch.uint8, device="cuda")
        self.sent_ln = torch.zeros((LINK_Q + LINK_B, P, n), dtype=torch.int32, device="cuda")

    def poll_and_compare(self, c, now, dg, ln, nonces, m_in, what, **tensors):
        """One poll on the device and in the model (m_in(h, s): the model's values of the optional
        inputs); state, outputs and sync datagram bytes compared.  Returns the model's outputs."""
        ep = self.ep
        ep.poll(self.mask, now, self.magic, dg, ln, nonces=torch.from_numpy(nonces.view(np.int32)).cuda(), **tensors)
        h_dg, h_ln = dg.cpu().numpy(), ln.cpu().numpy()
        got = {k: getattr(ep, k).cpu().numpy() for k in STATE_NAMES + OUT_NAMES + ("sync_datagrams",)}
        outs = {}
        for h in self.hs:
            for s in range(self.n):
                st = self.m_state[h][s]
                inp = {"call": c, "now": now, "magic": self.m_magic, "start": 0, "disconnected": 0, "ack_owed": 0, "reply_owed": 0,
                       "received": 0, "newest": NULL, "acked": NULL, "length": 0, "reports": 0,
                       "slots": [(int(h_ln[m, h, s]), h_dg[m, h, s].tobytes()) for m in range(h_ln.shape[0])],
                       "nonces": [int(x) for x in nonces[:, h, s]]}
                inp.update(m_in(h, s))
                o = outs[h, s] = model_step(st, inp, LINK_Q)
                where = f"{what}, endpoint ({h}, {s})"
                assert (got["ep_state"][h, s], got["sync_remaining"][h, s], got["sync_valid"][h, s], got["sync_next"][h, s],
                        got["packets_sent"][h, s], got["last_newest"][h, s], int(got["remote_magic"].view(np.uint16)[h, s])) == \
                    (st["state"], st["remaining"], st["valid"], st["next"], st["sent"], st["last_newest"], st["remote_magic"]), where
                assert got["sync_nonces"].view(np.uint32)[:, h, s].tolist() == st["nonces"], where
                assert got["stamps"][:, h, s].tolist() == [st[k] for k in STATE_ROW[4:9]], where
                assert (got["input_lengths"][h, s], got["ack_due"][h, s], got["reply_due"][h, s], got["report_due"][h, s],
                        got["keepalive_due"][h, s], got["sync_counts"][h, s], got["events_mask"][h, s], got["sync_count"][h, s],
                        got["liveness_received"][h, s], got["send_queue_len"][h, s], got["status"][h, s]) == \
                    (o["input_length"], o["ack_due"], o["reply_due"], o["report_due"], o["keepalive_due"], len(o["msgs"]), o["events"],
                     o["sync_count"], o["liveness"], o["queue"], o["status"]), where
                for m, data in enumerate(o["msgs"]):
                    assert got["sync_datagrams"][m, h, s, :16].tobytes() == data + bytes(6), where
                assert got["sync_lengths"][:, h, s].tolist() == [10] * len(o["msgs"]) + [0] * (LINK_Q - len(o["msgs"])), where
        want_run = np.array([all(outs[h, s]["synchronized"] for h in self.hs) for s in range(self.n)], np.uint8)
        assert np.array_equal(got["session_running"], want_run), what
        return outs


@pytest.mark.gpu
@pytest.mark.parametrize("P", [2, 4])
def test_gpu_two_batches_shake_hands_then_play_over_datagrams_only(gpu_available, P):
    """Two ex_game batches (S = 70; P = 2, and P = 4 with two local handles a side) that know only each
    other's address: distinct magics, remote_magic 0, a tenth of all datagrams lost, the handshake's
    included.  First the handshake: parse -> protocol -> build, the sync datagrams concatenated to
    build's along the slot axis, until every endpoint of both sides is Running (the caller holds every
    session in the lobby until then).  Then 60 calls of the whole frame loop, as test_datagram.py's
    match runs it but with the protocol deciding what is sent: export_local_inputs' `sent` is newest,
    the encoder's lengths go through poll to input_lengths, ack_due / reply_due / report_due /
    keepalive_due go to build, the peer's parse and decode give acked, reply_owed, received and
    ack_owed, and liveness takes liveness_received.  After every call the endpoint state and outputs
    and every datagram byte equal the models', the parse and the decode equal theirs, and each batch
    equals the oracles and a twin fed the true inputs directly."""
    from test_datagram import (FLIGHT_MS, MASK64, MATCH_SLOTS, MATCH_STRIDE, TICK_MS, Wire, model_build, model_parse,
                               report_words)
    from test_p2p_pacing import dev
    from test_wire_ring import LOOP_D, LOOP_STRIDE, SENT as RING_SENT, SL, W, Side, model_decode, model_encode
    assert SL == S
    half = (1 << (P // 2)) - 1
    masks = (half, half << (P // 2))
    rng = np.random.default_rng(0x5A5A + P)
    X = G.synth_inputs(S, P, PLAY_CALLS, seed=G.SEED ^ 0xD7, mask=0x0F, dtype=np.uint8)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ends = [Endpoints(P, m, S, 0x5A00 + i) for i, m in enumerate(masks)]
        pt = ends[0].pt
        # ---- the handshake
        parsed = [G.ParsedDatagrams(P, S, 64) for _ in masks]
        z = lambda shape, dt, v=0: torch.full(shape, v, dtype=dt, device="cuda")
        out_dg, out_ln = [z((LINK_B, P, S, STRIDE), torch.uint8) for _ in masks], [z((LINK_B, P, S), torch.int32) for _ in masks]
        cnt, bst, nulls, zeros8, zeros32 = z((P, S), torch.int32), z((P, S), torch.int32), z((P, S), torch.int32, NULL), \
            z((P, S), torch.uint8), z((P, S), torch.int32)
        now = EPOCH_MS
        for c in range(LOBBY_CAP):
            now += int(rng.integers(11, 22))      # 16 +- 5 ms: a uniform cadence would hold a lagging peer's retry off
            heard = []
            for i, e in enumerate(ends):
                lost = rng.random((LINK_Q + LINK_B, P, S)) < 0.1
                peer = ends[1 - i]
                heard.append((peer.sent_dg[:, pt].contiguous(),
                              (peer.sent_ln[:, pt] * torch.from_numpy((~lost).astype(np.int32)).cuda()).contiguous()))
            for i, e in enumerate(ends):
                dg, ln = heard[i]
                G.parse_datagrams(parsed[i], e.mask, dg, ln, e.ep.remote_magic, now)
                h_recv, h_owed = parsed[i].received.cpu().numpy(), parsed[i].reply_owed.cpu().numpy()
                start = z((P, S), torch.uint8, 1 if c == 0 else 0)
                nonces = rng.integers(0, 2**32, (LINK_Q + LINK_B, P, S), dtype=np.uint32)
                e.poll_and_compare(c, now, dg, ln, nonces,
                                   lambda h, s: {"start": int(c == 0), "reply_owed": int(h_owed[h, s]), "received": int(h_recv[h, s])},
                                   f"handshake call {c}, side {i}", start=start, reply_owed=parsed[i].reply_owed,
                                   received=parsed[i].received)
                G.build_datagrams(e.mask, out_dg[i], out_ln[i], cnt, bst, e.magic, now, nulls, nulls, zeros8, reply_owed=e.ep.reply_due,
                                  reply_ping=parsed[i].reply_ping, report_due=e.ep.report_due, frame_advantage=zeros32,
                                  keepalive_due=e.ep.keepalive_due)
                e.sent_dg = torch.cat([e.ep.sync_datagrams, out_dg[i]])
                e.sent_ln = torch.cat([e.ep.sync_lengths, out_ln[i]])
            if all(st["state"] == RUNNING for e in ends for h in e.hs for st in e.m_state[h]):
                print(f"P = {P}: every endpoint Running after {c + 1} calls")
                break
        else:
            raise AssertionError("a pair is still shaking hands")
        for i, e in enumerate(ends):      # everyone learned the peer's magic
            assert all(st["remote_magic"] == ends[1 - i].m_magic for h in e.hs for st in e.m_state[h])
        # ---- the match
        sides = [Side(G.Game.EX_GAME, P, m, S, np.uint8, stream) for m in masks]
        for side in sides:
            for b in (side.sess, side.twin):
                b.enable_liveness()
        wires = [Wire(P, m, S, 1, e.m_magic) for m, e in zip(masks, ends)]
        for w in wires:
            w.ack_dev, w.m_ack = z((P, S), torch.uint8), np.zeros((P, S), np.uint8)
        dx = dev(X)
        base = now
        inputs_sent = 0
        for t in range(PLAY_CALLS):
            now = base + TICK_MS * (t + 1)
            for i in (0, 1):
                wire, side, peer, back, e = wires[i], sides[i], sides[1 - i], wires[1 - i], ends[i]
                link, hs = wire.link, wire.hs
                what = f"hop {'AB'[i]} -> {'BA'[i]}, tick {t}"
                side.exported(link, what)
                acked, m_acked = link.acked()
                side.ring.send_packets(link.mask, link.sent, acked, LOOP_D, link.pk, link.ln, link.st)
                want = model_encode(side.m_ring, link.mask, m_acked, link.m_sent, LOOP_D, LOOP_STRIDE)
                assert (want[1][hs] >= 0).all(), what
                ack_frame, m_ack = side.ring.upto[pt].contiguous(), side.m_upto[pt]
                # the protocol: what this side heard (the opposite wire, as its hop left it) and what it has to send
                nonces = rng.integers(0, 2**32, (MATCH_SLOTS, P, S), dtype=np.uint32)
                outs = e.poll_and_compare(
                    LOBBY_CAP + t, now, back.dg[:, pt].contiguous(), back.ln[:, pt].contiguous(), nonces,
                    lambda h, s: {"ack_owed": int(back.m_ack[pt[h], s]), "reply_owed": int(back.m_owed[pt[h], s]),
                                  "received": int(back.m_received[pt[h], s]), "newest": int(link.m_sent[h, s]),
                                  "acked": int(m_acked[h, s]), "length": int(want[1][h, s])},
                    what, ack_owed=back.ack_dev[pt].contiguous(), reply_owed=back.parsed.reply_owed[pt].contiguous(),
                    received=back.parsed.received[pt].contiguous(), newest=link.sent, acked=acked, lengths=link.ln)
                ep = e.ep
                e.m_live = np.zeros((P, S), np.uint8)       # the model's liveness_received, in the remote handle's row
                for (h, s), o in outs.items():
                    e.m_live[pt[h], s] = o["liveness"]
                G.build_datagrams(link.mask, wire.dg, wire.ln, wire.cnt, wire.st, wire.magic, now, ack_frame, wire.no_last, wire.no_disc,
                                  packets=link.pk, lengths=ep.input_lengths, start_frames=link.st, ack_owed=ep.ack_due,
                                  reply_owed=ep.reply_due, reply_ping=back.parsed.reply_ping[:, pt].contiguous(),
                                  report_due=ep.report_due, frame_advantage=wire.parsed.frame_advantage * 0,
                                  keepalive_due=ep.keepalive_due)
                dg, ln = wire.dg.cpu().numpy(), wire.ln.cpu().numpy()
                sent = {}
                for h in hs:
                    for s in range(S):
                        o = outs[h, s]
                        b = {"magic": wire.m_magic, "now": now, "length": o["input_length"], "start": int(want[2][h, s]),
                             "ack": int(m_ack[h, s]), "requested": 0, "last": [NULL] * P, "disc": [0] * P, "ack_owed": o["ack_due"],
                             "reply_owed": o["reply_due"], "ping": int(back.m_ping[pt[h], s]), "report_due": o["report_due"],
                             "advantage": 0, "keepalive": o["keepalive_due"], "reports": [], "packet": want[0].get((h, s), b"")}
                        msgs, status = model_build(b, P, MATCH_SLOTS, MATCH_STRIDE, LOOP_STRIDE)
                        where = f"{what}, ({h}, {s})"
                        assert status == 0 and ln[:, h, s].tolist() == [len(m) for m in msgs] + [0] * (MATCH_SLOTS - len(msgs)), where
                        for k, m in enumerate(msgs):
                            assert dg[k, h, s, :len(m)].tobytes() == m, f"{where}, datagram {k}"
                        sent[h, s] = msgs
                        inputs_sent += int(o["input_length"] > 0)
                keep = ~(rng.random((MATCH_SLOTS, P, S)) < 0.1)
                wire.ln.mul_(torch.from_numpy(keep.astype(np.int32)).cuda())
                heard_at = now + FLIGHT_MS
                G.parse_datagrams(wire.parsed, link.mask, wire.dg, wire.ln, peer_magic(ends[1 - i], pt), heard_at)
                got = {k: v.cpu().numpy() for k, v in wire.parsed.tensors().items()}
                m_pk = np.zeros((P, S, LOOP_STRIDE), np.uint8)
                m_ln, m_st = np.zeros((P, S), np.int32), np.zeros((P, S), np.int32)
                m_acks = np.full((P, S), NULL, np.int32)
                for h in hs:
                    for s in range(S):
                        msgs = sent[h, s] + [b""] * (MATCH_SLOTS - len(sent[h, s]))
                        slots = [(len(msgs[m]) * int(keep[m, h, s]), msgs[m] + bytes(MATCH_STRIDE - len(msgs[m]))) for m in range(MATCH_SLOTS)]
                        st = wire.m_state[h][s]
                        o = model_parse(st, slots, wire.m_magic, heard_at, P, MATCH_STRIDE, LOOP_STRIDE)
                        where = f"{what}, ({h}, {s})"
                        assert (got["received"][h, s], got["status"][h, s], got["lengths"][h, s], got["start_frames"][h, s]) == \
                            (o["received"], o["status"], o["length"], o["start"]), where
                        assert got["acked"][h, s] == st["acked"], where
                        assert got["packets"][h, s, :o["length"]].tobytes() == o["packet"], where
                        assert (got["frame_advantage"][h, s], got["rtt_ms"][h, s], got["reply_owed"][h, s]) == \
                            (st["advantage"], st["rtt"], o["owed"]), where
                        assert (int(got["reply_ping"][0, h, s]), int(got["reply_ping"][1, h, s])) == (o["ping"] & MASK64, o["ping"] >> 64), where
                        m_pk[h, s, :o["length"]] = np.frombuffer(o["packet"], np.uint8)
                        m_ln[h, s], m_st[h, s], m_acks[h, s] = o["length"], o["start"], st["acked"]
                        wire.m_received[h, s], wire.m_owed[h, s], wire.m_ping[h, s] = o["received"], o["owed"], o["ping"] & MASK64
                peer.ring.receive_packets(link.mask, wire.parsed.packets, wire.parsed.lengths, wire.parsed.start_frames, W, status=link.status)
                m_status = np.full((P, S), RING_SENT, np.int32)
                model_decode(peer.m_ring, peer.m_upto, m_status, link.mask, m_pk, m_ln, m_st)
                np.testing.assert_array_equal(link.status.cpu().numpy()[hs], m_status[hs], err_msg=f"decode status, {what}")
                np.testing.assert_array_equal(peer.ring.upto.cpu().numpy()[hs], peer.m_upto[hs], err_msg=f"upto, {what}")
                assert (m_status[hs] >= 0).all(), what
                # on_input queues an InputAck for every Input it could decode (:653-682)
                wire.ack_dev = ((wire.parsed.lengths > 0) & (link.status >= 0)).to(torch.uint8)
                wire.m_ack = ((m_ln > 0) & (m_status >= 0)).astype(np.uint8)
                back.link.push(wire.parsed.acked[pt].contiguous(), m_acks[pt])
            for i, side in enumerate(sides):
                peer, heard_w, e = sides[1 - i], wires[1 - i], ends[i]
                side.sess.poll_liveness(now, e.ep.liveness_received[pt].contiguous(), heard_w.parsed.disconnect_requested)
                side.twin.poll_liveness(now, torch.from_numpy(e.m_live).cuda())
                side.tick(t, X, dx, lambda h: peer.truth[:, h], f"side {'AB'[i]}, tick {t}")
                for x, y in zip(side.sess.read_liveness(), side.twin.read_liveness()):
                    assert np.array_equal(x, y), f"liveness, side {'AB'[i]}, tick {t}"
        assert inputs_sent > PLAY_CALLS * S * P // 2     # an Input is due whenever the tick queued a new frame
        assert all((s.sess.frames()[0] > PLAY_CALLS // 2).all() for s in sides) and all(s.sess.counters()[2] == 0 for s in sides)
        assert all(s.sess.network_events()[0].sum() == 0 for s in sides)
        for s in sides:
            s.close()


def peer_magic(end, pt):
    """The remote_magic rows a parse of the peer's wire filters by: what the hearing side's endpoints learned."""
    return end.ep.remote_magic[pt].contiguous()
