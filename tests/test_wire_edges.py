"""The packet codec (network/compression.rs: XOR delta + bitfield RLE) at its format edges.

tests/test_wire.py pins the codec on the packets a hold-model stream of small inputs makes:
1-byte headers, zero runs, short literals.  Here are the edges of the format itself — 0xFF
runs, 2-byte run and literal headers, the 65,536-byte run limit, padded and over-wide
LEB128 headers, streams that end inside an input, encoder overflow — first as a vector
table pinned by hand and checked on the oracle (CPU), then on the stand-alone kernels
(rb_encode_input_packets / rb_decode_input_packets, input sizes 1, 2 and 4) and on the
decoder inside the P2P tick (rb_p2p_run_ticks_packets, ex_game's 1-byte and the stub
game's 4-byte inputs).  The oracle is the expectation everywhere.

Every malformed vector is one the decoders reject from bytes inside its own length: a
header is read only while pos < n, a literal only after len <= n - pos.
"""
import numpy as np
import pytest

from oracle import oracle as O
from test_wire import on_input_reference

REFS = {1: bytes([0x5A]), 2: bytes([0x5A, 0xC3]), 4: bytes([0x5A, 0xC3, 0x0F, 0xF0])}


def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def run(n, ff=False):
    return varint((n << 2) | (2 if ff else 0) | 1)


def lit(b):
    return varint(len(b) << 1) + bytes(b)


L63 = bytes(range(1, 64))
L64 = bytes(range(1, 65))
AB = bytes([0xAA, 0xBB, 0xCC, 0xDD])

# (name, packet bytes, the RLE-decoded XOR stream written out by hand; None: malformed).
# The packets are spelled in hex where the header is the point of the vector.
STREAMS = [
    ("zero_run_4", bytes([0x11]), b"\x00" * 4),
    ("ff_run_4", bytes([0x13]), b"\xff" * 4),
    ("zero_run_31", bytes([0x7D]), b"\x00" * 31),           # partial input for ib 2 and 4
    ("ff_run_31", bytes([0x7F]), b"\xff" * 31),
    ("zero_run_28", bytes([0x71]), b"\x00" * 28),           # the longest 1-byte-header run of whole u32s
    ("ff_run_28", bytes([0x73]), b"\xff" * 28),
    ("zero_run_32", bytes([0x81, 0x01]), b"\x00" * 32),     # 2-byte header
    ("ff_run_32", bytes([0x83, 0x01]), b"\xff" * 32),
    ("zero_run_33", bytes([0x85, 0x01]), b"\x00" * 33),
    ("ff_run_33", bytes([0x87, 0x01]), b"\xff" * 33),
    ("ff_run_36", bytes([0x93, 0x01]), b"\xff" * 36),
    ("literal_63", bytes([0x7E]) + L63, L63),
    ("literal_64", bytes([0x80, 0x01]) + L64, L64),         # 2-byte literal header
    ("literal_60", bytes([0x78]) + L63[:60], L63[:60]),
    ("lit_ffrun_lit", bytes([0x08]) + AB + bytes([0x23]) + bytes([0x08]) + AB[::-1], AB + b"\xff" * 8 + AB[::-1]),
    ("lit_ffrun_lit_odd", bytes([0x06, 1, 2, 3, 0x17, 0x02, 4]), bytes([1, 2, 3]) + b"\xff" * 5 + bytes([4])),
    ("run_65536", bytes([0x81, 0x80, 0x10]), b"\x00" * 65536),
    ("ff_run_65536", bytes([0x83, 0x80, 0x10]), b"\xff" * 65536),
    ("run_65537", bytes([0x85, 0x80, 0x10]), None),
    ("literal_longer_than_data", bytes([0x0A, 1, 2, 3, 4]), None),
    ("truncated_varint", bytes([0x80]), None),
    ("truncated_varint_after_run", bytes([0x11, 0x88, 0x80]), None),
    # a 5-byte header whose bits 32-34 are set: a literal of 2^31 + 2 bytes / a run of 2^30
    ("varint_bit32_literal", bytes([0x88, 0x80, 0x80, 0x80, 0x10]) + AB, None),
    ("varint_bit32_run", bytes([0x81, 0x80, 0x80, 0x80, 0x10]), None),
    ("varint_bit34_run", bytes([0x91, 0x80, 0x80, 0x80, 0x40]), None),
    # headers padded with zero continuation groups (non-canonical): 6 and 10 bytes
    ("varint_padded6_literal", bytes([0x88, 0x80, 0x80, 0x80, 0x80, 0x00]) + AB, AB),
    ("varint_padded6_run", bytes([0x91, 0x80, 0x80, 0x80, 0x80, 0x00]), b"\x00" * 4),
    ("varint_padded10_literal", bytes([0x88] + [0x80] * 8 + [0x00]) + AB, AB),
    ("varint_padded10_dropped_bits", bytes([0x88] + [0x80] * 8 + [0x7E]) + AB, AB),  # bits past bit 63 are dropped
    ("varint_bit63", bytes([0x88] + [0x80] * 8 + [0x01]) + AB, None),
    ("varint_bit35", bytes([0x88, 0x80, 0x80, 0x80, 0x80, 0x01]) + AB, None),
    ("varint_11_bytes", bytes([0x88] + [0x80] * 9 + [0x00]) + AB, None),
    ("literal_3", bytes([0x06, 1, 2, 3]), bytes([1, 2, 3])),   # ends inside an input for ib 2 and 4
    ("zero_run_6", bytes([0x19]), b"\x00" * 6),               # whole inputs for ib 1 and 2 only
    ("zero_length_run", bytes([0x01]), b""),
    ("empty_literal", bytes([0x00]), b""),
    ("empty_literal_then_run", bytes([0x00, 0x13]), b"\xff" * 4),
    # more frames than an InputQueue holds, in 2 bytes: 800 zero bytes
    ("zero_run_800", bytes([0x81, 0x19]), b"\x00" * 800),
]


def table():
    """(name, ib, ref, packet, expected inputs [n, ib] as a uint8 array; None: malformed)."""
    rows = []
    for ib in (1, 2, 4):
        ref = REFS[ib]
        for name, packet, stream in STREAMS:
            if stream is None or len(stream) % ib:
                want = None  # compression.rs:47: the delta decoder asserts whole inputs
            else:
                want = (np.frombuffer(stream, np.uint8).reshape(-1, ib) ^ np.frombuffer(ref, np.uint8)[None, :])
            rows.append((f"{name}-ib{ib}", ib, ref, packet, want))
    return rows


TABLE = table()


def test_vector_table_is_what_the_oracle_decodes():
    assert len({r[0] for r in TABLE}) == len(TABLE) == 3 * len(STREAMS)
    verdicts = {}
    for name, ib, ref, packet, want in TABLE:
        got = O.wire_decode(ref, packet, cap=70000)
        if want is None:
            assert got is None, name
        else:
            assert got is not None, name
            np.testing.assert_array_equal(got, want, err_msg=name)
        verdicts[name] = got is not None
    # the headline verdicts, spelled out
    assert not verdicts["varint_bit32_literal-ib1"] and not verdicts["varint_bit32_run-ib1"]
    assert verdicts["varint_padded6_literal-ib1"] and verdicts["varint_padded6_run-ib4"]
    assert verdicts["run_65536-ib4"] and not verdicts["run_65537-ib1"]
    assert verdicts["zero_run_6-ib2"] and not verdicts["zero_run_6-ib4"] and not verdicts["literal_3-ib2"]
    assert O.wire_decode(REFS[1], bytes([0x84, 0x80, 0x80, 0x80, 0x10, 0xAA, 0xBB])) is None
    assert O.wire_decode(b"\0", bytes([0x84, 0x80, 0x80, 0x80, 0x80, 0x00, 0xAA, 0xBB])).tolist() == [[0xAA], [0xBB]]


def segments(packet):
    """[(kind, position, header bytes, length)] of a well-formed packet; kind 'lit', 'run0' or 'runf'."""
    out, p = [], 0
    while p < len(packet):
        p0, v, sh = p, 0, 0
        while True:
            b = packet[p]
            p += 1
            v |= (b & 0x7F) << sh
            sh += 7
            if not b & 0x80:
                break
        if v & 1:
            out.append(("runf" if v & 2 else "run0", p0, p - p0, v >> 2))
        else:
            out.append(("lit", p0, p - p0, v >> 1))
            p += v >> 1
    assert p == len(packet)
    return out


def block_stream(rng, n, ib, lo=4, hi=40):
    """n inputs in held blocks of lo..hi frames: a base value v, ~v (against v as the reference
    the XOR stream is a 0xFF run), zero, all ones, or a fresh value."""
    v = rng.integers(0, 256, ib, dtype=np.uint8)
    out = np.empty((n, ib), np.uint8)
    i = 0
    while i < n:
        k = int(rng.integers(lo, hi + 1))
        c = rng.random()
        val = v if c < 0.3 else ~v if c < 0.6 else rng.integers(0, 256, ib, dtype=np.uint8) if c < 0.9 else \
            np.full(ib, 0xFF if c < 0.95 else 0, np.uint8)
        out[i:i + k] = val
        i += k
    return out


@pytest.mark.parametrize("ib", [1, 2, 4])
def test_round_trips_of_full_byte_holds(ib):
    rng = np.random.default_rng(40 + ib)
    kinds = set()
    for _ in range(300):
        n = int(rng.integers(1, 120))
        ins = block_stream(rng, n + 1, ib)
        ref = ins[0].tobytes()
        enc = O.wire_encode(ref, ins[1:])
        np.testing.assert_array_equal(O.wire_decode(ref, enc), ins[1:])
        kinds |= {(k, h) for k, _, h, _ in segments(enc)}
    assert {("runf", 1), ("runf", 2), ("run0", 1), ("run0", 2), ("lit", 1), ("lit", 2)} <= kinds


# ---------------------------------------------------------------------------- the stand-alone kernels
def _encode_case(ib, S=3000, F=160, seed=0):
    rng = np.random.default_rng(seed + ib)
    dt = {1: np.uint8, 2: np.uint16, 4: np.uint32}[ib]
    P, h = 2, 1
    raw = np.zeros((F, P, S, ib), np.uint8)
    for s in range(S):
        raw[:, h, s] = block_stream(rng, F, ib)
    acked = rng.integers(-1, 50, S).astype(np.int32)
    newest = (acked + rng.integers(0, 101, S)).astype(np.int32)
    want = []
    for s in range(S):
        if newest[s] <= acked[s]:
            want.append(b"")
            continue
        ref = bytes(ib) if acked[s] == -1 else raw[acked[s], h, s].tobytes()
        want.append(O.wire_encode(ref, raw[acked[s] + 1:newest[s] + 1, h, s]))
    return dt, P, h, raw, acked, newest, want


def _tight_stride(want):
    """A row length at which packets fit exactly, overflow by one byte, and overflow inside a
    segment header (the byte at the row's end is a header byte): the one with the most of the
    rarest kind."""
    lens = np.array([len(w) for w in want])
    hdr_at = {}
    for w in want:
        for _, p0, hb, _ in segments(w):
            for q in range(p0, p0 + hb):
                hdr_at[q] = hdr_at.get(q, 0) + 1
    best = max(range(8, 200), key=lambda L: min((lens == L).sum(), (lens == L + 1).sum(), hdr_at.get(L, 0)))
    return best


@pytest.mark.gpu
@pytest.mark.parametrize("ib", [1, 2, 4])
def test_gpu_encoder_at_the_format_edges(gpu_available, ib):
    import ctypes

    import torch

    from ggrs_amd import _lib as L
    lib = L.load()
    S, F = 3000, 160
    dt, P, h, raw, acked, newest, want = _encode_case(ib, S, F)
    segs = [sg for w in want for sg in segments(w)]
    assert any(k == "runf" and hb == 1 for k, _, hb, _ in segs), "no 0xFF run with a 1-byte header"
    assert any(k == "runf" and hb == 2 for k, _, hb, _ in segs), "no 0xFF run with a 2-byte header"
    assert any(k == "lit" and hb == 2 for k, _, hb, _ in segs), "no literal of 64 bytes or more"
    lens = np.array([len(w) for w in want])
    roomy = int(lens.max()) + 8
    tight = _tight_stride(want)
    fits, by_one = int((lens == tight).sum()), int((lens == tight + 1).sum())
    at_header = sum(1 for w in want if len(w) > tight and any(p0 <= tight < p0 + hb for _, p0, hb, _ in segments(w)))
    assert fits > 0 and by_one > 0 and at_header > 0, (tight, fits, by_one, at_header)
    d_in = torch.from_numpy(raw.reshape(F, P, S * ib).view(dt).reshape(F, P, S)).cuda()
    d_ack, d_new = torch.from_numpy(acked).cuda(), torch.from_numpy(newest).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for stride in (roomy, tight):
        guard = 64  # bytes past the last row: an overflowing lane must not write there either
        pk = torch.full((S * stride + guard,), 0xEE, dtype=torch.uint8, device="cuda")
        ln = torch.zeros(S, dtype=torch.int32, device="cuda")
        st = torch.zeros(S, dtype=torch.int32, device="cuda")
        assert lib.rb_encode_input_packets(0, None, h, P, S, ib, p(d_in), F, 0, p(d_ack), p(d_new), p(pk), stride,
                                           p(ln), p(st)) == 0
        torch.cuda.synchronize()
        pk_h, ln_h, st_h = pk.cpu().numpy(), ln.cpu().numpy(), st.cpu().numpy()
        assert (pk_h[S * stride:] == 0xEE).all()
        pk_h = pk_h[:S * stride].reshape(S, stride)
        np.testing.assert_array_equal(st_h, acked + 1)
        over = lens > stride
        assert over.any() == (stride == tight)
        np.testing.assert_array_equal(ln_h == -1, over, err_msg=f"overflow lanes, stride {stride}")
        for s in np.nonzero(~over)[0]:
            assert ln_h[s] == lens[s], (s, ln_h[s], lens[s])
            assert pk_h[s, :lens[s]].tobytes() == want[s], s
            assert (pk_h[s, lens[s]:] == 0xEE).all(), s  # nothing written past the packet


@pytest.mark.gpu
@pytest.mark.parametrize("ib", [1, 2, 4])
def test_gpu_decoder_on_every_vector(gpu_available, ib):
    """Every vector of the table in a lane of its own, under three receiver states: nothing received
    yet (blank reference), two frames of the packet already received, and a packet that starts two
    frames below remote_frames (the decoder clips there: the guard frames above stay untouched and
    the newest frame stops at the last one written)."""
    import ctypes

    import torch

    from ggrs_amd import _lib as L
    lib = L.load()
    rows = [r for r in TABLE if r[1] == ib]
    V = len(rows)
    stride = 96
    assert max(len(r[3]) for r in rows) <= stride
    P, h, W, RF, GUARD = 2, 1, 8, 40, 8
    states = [(-1, 0), (11, 10), (RF - 3, RF - 2)]  # (last received, the packet's start frame)
    S = V * len(states)
    rng = np.random.default_rng(7 + ib)
    recv = rng.integers(0, 256, (RF + GUARD, P, S, ib), dtype=np.uint8)  # every frame the packet leaves must stay
    pk = np.zeros((S, stride), np.uint8)
    lens = np.zeros(S, np.int32)
    start = np.zeros(S, np.int32)
    last = np.zeros(S, np.int32)
    for i, (ls, stf) in enumerate(states):
        for v, (_, _, ref, packet, _) in enumerate(rows):
            s = i * V + v
            pk[s, :len(packet)] = np.frombuffer(packet, np.uint8)
            lens[s], start[s], last[s] = len(packet), stf, ls
            if ls != -1:
                recv[stf - 1, h, s] = np.frombuffer(ref, np.uint8)
    upto = np.full((P, S), -1, np.int32)
    upto[h] = last
    dt = {1: np.uint8, 2: np.uint16, 4: np.uint32}[ib]
    d_recv = torch.from_numpy(recv.reshape(RF + GUARD, P, S * ib).view(dt).reshape(RF + GUARD, P, S)).cuda()
    d_upto = torch.from_numpy(upto).cuda()
    d_pk, d_len, d_start = (torch.from_numpy(a).cuda() for a in (pk, lens, start))
    d_st = torch.full((S,), 77, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.rb_decode_input_packets(0, None, h, P, S, ib, W, p(d_pk), stride, p(d_len), p(d_start), p(d_recv), RF,
                                       p(d_upto), p(d_st)) == 0
    torch.cuda.synchronize()
    got = d_recv.cpu().numpy().view(np.uint8).reshape(RF + GUARD, P, S, ib)
    got_upto, got_st = d_upto.cpu().numpy(), d_st.cpu().numpy()
    want_recv = recv.copy()
    codes = set()
    for s in range(S):
        name, _, ref, packet, want = rows[s % V]
        refin = bytes(ib) if last[s] == -1 else ref
        out, nl, code = on_input_reference(int(last[s]), int(start[s]), packet, refin, W, ib)
        if want is None:
            assert code == -1, name
        out = {f: b for f, b in out.items() if f < RF}  # the caller's tensor ends at remote_frames
        nl = max(out) if out else int(last[s])
        if code == 0 and not out:
            code = 1
        codes.add(code)
        assert got_st[s] == code, (name, s, got_st[s], code)
        assert got_upto[h, s] == nl, (name, s, got_upto[h, s], nl)
        for f, b in out.items():
            want_recv[f, h, s] = np.frombuffer(b, np.uint8)
    np.testing.assert_array_equal(got_upto[0], upto[0])
    np.testing.assert_array_equal(got, want_recv)  # the written inputs, and every other byte untouched (guards, neighbours)
    assert codes == {0, 1, -1}


# ---------------------------------------------------------------------------- the decoder inside the P2P tick
def _start(game, S, P, W, rd, mask):
    import ggrs_amd as G
    from ggrs_amd.p2p import PlayerType
    b = (G.SessionBuilder(game, num_sessions=S).with_num_players(P).with_max_prediction_window(W)
         .with_input_delay(1).with_remote_input_delay(rd))
    for hh in range(P):
        b.add_player(PlayerType.Local if (mask >> hh) & 1 else PlayerType.Remote, hh)
    return b.start_p2p_session()


def run_packets_against_oracle(wired, orc, P, mask, inputs, pk, ln, st, uptos, recvs, codes, chunks, dead_at=None):
    """The calls of `chunks` ticks on the packet-fed batch and the same ticks on the oracle, which is
    delivered what UdpProtocol::on_input's restatement decoded (_oracle_packet_deliveries).  After every
    call: status, rollback frame, request counts, decode statuses, acks, cells, states and queues.
    dead_at {session: tick}: the packet of that tick is one the reference panics on while decoding
    (status -1); the oracle has no decoder, so that session is expected to stop there with RB_PANIC.
    A session the oracle itself panics (its InputQueue's asserts) must stop on the device too.  A
    stopped session keeps the decode status of the tick that stopped it.  Returns the sessions alive."""
    import torch

    from ggrs_amd._lib import RB_PANIC
    from test_p2p import compare_state
    S = inputs.shape[2]
    di = torch.from_numpy(inputs).cuda()
    dstat = torch.zeros((P, S), dtype=torch.int32, device="cuda")
    acks = torch.full((P, S), -1, dtype=torch.int32, device="cuda")
    remotes = [hh for hh in range(P) if not (mask >> hh) & 1]
    died = np.full(S, -1, np.int64)  # the tick that stopped the session
    t = 0
    for n in chunks:
        wired.run_ticks_packets(di[t:t + n], pk[t:t + n], ln[t:t + n], st[t:t + n], dstat, acks)
        for k in range(t, t + n):
            for hh in remotes:
                orc.deliver(hh, uptos[k, hh], recvs[k][:, hh, :])
            for hh in range(P):
                if (mask >> hh) & 1:
                    orc.add_local_input(hh, inputs[k, hh])
            ost, olf, ona, ons = orc.advance()
            stop = ost == O.KIND_PANIC
            for s_, tk in (dead_at or {}).items():
                stop[s_] |= tk <= k
            died = np.where((died < 0) & stop, k, died)
        t += n
        alive = died < 0
        got_st, lf, na, ns = wired.status()
        differ = np.nonzero((got_st == RB_PANIC) != ~alive)[0]
        assert differ.size == 0, (f"tick {t - 1}: sessions {differ.tolist()} stopped on one side only "
                                  f"(device {got_st[differ].tolist()}, oracle {ost[differ].tolist()}: {orc.last_panic()})")
        np.testing.assert_array_equal(got_st[alive], ost[alive], err_msg=f"status, tick {t - 1}")
        np.testing.assert_array_equal(lf[alive], olf[alive], err_msg=f"LoadGameState frame, tick {t - 1}")
        np.testing.assert_array_equal(na[alive], ona[alive], err_msg=f"AdvanceFrame count, tick {t - 1}")
        np.testing.assert_array_equal(ns[alive], ons[alive], err_msg=f"SaveGameState count, tick {t - 1}")
        at = np.where(alive, t - 1, died)
        want_ds = codes[at[None, :], np.array(remotes)[:, None], np.arange(S)[None, :]]
        np.testing.assert_array_equal(dstat.cpu().numpy()[remotes], want_ds, err_msg=f"decode status, tick {t - 1}")
        np.testing.assert_array_equal(acks.cpu().numpy()[remotes][:, alive], uptos[t - 1][remotes][:, alive],
                                      err_msg=f"acks, tick {t - 1}")
        compare_state(wired, orc, t - 1, alive)
    assert t == inputs.shape[0]
    assert wired.counters()[2] == int((died >= 0).sum())
    return died < 0


FORMS = (1,) * 35 + (7, 8, 30)  # one tick per launch, 4-23 ticks (input ring in LDS), >= 24 ticks (LDS cells)


def full_byte_block_network(S, T, rd):
    """ex_game, P 2, handle 1 remote, on the full-byte stream; in every other session the remote player
    holds v and ~v alternately in blocks of 4-40 frames, so a packet that starts at a block's edge is a
    single 0xFF run and one inside a block a zero run of up to 33 bytes."""
    from ggrs_amd.p2p import synth_network
    inputs, upto, rin = synth_network(S, 2, T, 0b01, rd, 1, 5, mask=0xFF)
    rng = np.random.default_rng(77)
    for s in range(0, S, 2):
        v = np.uint8(inputs[0, 1, s])
        t, k = 0, 0
        while t < T:
            n = int(rng.integers(4, 41))
            inputs[t:t + n, 1, s] = v if k % 2 == 0 else ~v
            t, k = t + n, k + 1
    rin[rd:] = inputs
    return inputs, upto, rin


def assert_schedule_covers_the_edges(pk, ln):
    """On the CPU, before the ticks run: the schedule holds single-header 0xFF-run packets (the
    fast path's `run` with fill 0xFF), zero and 0xFF runs with 2-byte headers, packets of exactly
    32 and 33 bytes, and multi-segment packets past 32 bytes."""
    pk_h, ln_h = pk.cpu().numpy(), ln.cpu().numpy()
    seen = {"ff1": 0, "run2": 0, "n32": 0, "n33": 0, "multi": 0}
    for idx in zip(*np.nonzero(ln_h > 0)):
        n = int(ln_h[idx])
        sg = segments(pk_h[idx][:n].tobytes())
        seen["ff1"] += n == 1 and sg[0][0] == "runf"
        seen["run2"] += any(k != "lit" and hb == 2 for k, _, hb, _ in sg)
        seen["n32"] += n == 32
        seen["n33"] += n == 33
        seen["multi"] += n > 32 and len(sg) > 1
    assert all(v > 0 for v in seen.values()), seen
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("lockstep", [False, True], ids=["async", "lockstep"])
def test_gpu_packet_ticks_on_full_byte_blocks_match_oracle(gpu_available, monkeypatch, lockstep):
    import torch

    import ggrs_amd as G
    from ggrs_amd import _lib as L
    from test_wire import _encode_schedule, _oracle_packet_deliveries
    monkeypatch.setenv("RB_P2P_SYNC_TICKS", "1" if lockstep else "0")
    lib = L.load()
    S, P, mask, rd, W, stride, max_redo = 200, 2, 0b01, 1, 16, 64, 32
    T = sum(FORMS)
    inputs, upto, rin = full_byte_block_network(S, T, rd)
    pk, ln, st = _encode_schedule(lib, P, S, T, mask, rd, upto, torch.from_numpy(rin).cuda(), stride, seed=3,
                                  max_redo=max_redo)
    assert_schedule_covers_the_edges(pk, ln)
    uptos, recvs, codes = _oracle_packet_deliveries(P, S, T, mask, W, rin.shape[0], pk, ln, st)
    assert (codes >= 0).all()
    np.testing.assert_array_equal(uptos[-1][1], upto[-1][1])
    got = np.arange(rin.shape[0])[:, None] <= uptos[-1][1][None, :]  # the oracle's decode of the packets: the stream
    np.testing.assert_array_equal(recvs[-1][:, 1][got], rin[:, 1][got])
    wired = _start(G.Game.EX_GAME, S, P, W, rd, mask)
    orc = O.OracleP2P(O.EX_GAME, P, W, 1, mask, S, sparse_saving=False, remote_delay=rd)
    alive = run_packets_against_oracle(wired, orc, P, mask, inputs, pk, ln, st, uptos, recvs, codes, FORMS)
    assert alive.all() and wired.totals()[2] > 0
    wired.close()
    orc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lockstep", [False, True], ids=["async", "lockstep"])
def test_gpu_packet_ticks_of_u32_inputs_match_oracle(gpu_available, monkeypatch, lockstep):
    """The stub game: 4-byte inputs, any u32.  Re-sent windows of up to 6 frames make packets past the
    fast paths (literal + zero run + literal at 4 bytes per input)."""
    import torch

    import ggrs_amd as G
    from ggrs_amd import _lib as L
    from ggrs_amd.p2p import synth_network
    from test_wire import _encode_schedule, _oracle_packet_deliveries
    monkeypatch.setenv("RB_P2P_SYNC_TICKS", "1" if lockstep else "0")
    lib = L.load()
    S, P, mask, rd, W, stride, max_redo = 200, 2, 0b01, 1, 8, 64, 6
    T = sum(FORMS)
    inputs, upto, rin = synth_network(S, P, T, mask, rd, 1, 5, dtype=np.uint32, mask=0xFFFFFFFF)
    assert (rin[rd:, 1] >= 1 << 24).mean() > 0.9
    pk, ln, st = _encode_schedule(lib, P, S, T, mask, rd, upto, torch.from_numpy(rin).cuda(), stride, seed=4,
                                  max_redo=max_redo, ib=4)
    pk_h, ln_h = pk.cpu().numpy(), ln.cpu().numpy()
    multi = sum(len(segments(pk_h[i][:ln_h[i]].tobytes())) > 1 for i in zip(*np.nonzero(ln_h > 0)))
    assert multi > S and int(ln_h.max()) > 32, (multi, int(ln_h.max()))  # the general decoder, past the 32-byte window
    uptos, recvs, codes = _oracle_packet_deliveries(P, S, T, mask, W, rin.shape[0], pk, ln, st, ib=4)
    assert (codes >= 0).all()
    got = np.arange(rin.shape[0])[:, None] <= uptos[-1][1][None, :]  # the oracle's decode of the packets: the stream
    np.testing.assert_array_equal(recvs[-1][:, 1][got], rin[:, 1][got])
    wired = _start(G.Game.STUB, S, P, W, rd, mask)
    orc = O.OracleP2P(O.STUB, P, W, 1, mask, S, sparse_saving=False, remote_delay=rd)
    alive = run_packets_against_oracle(wired, orc, P, mask, inputs, pk, ln, st, uptos, recvs, codes, FORMS)
    assert alive.all() and wired.totals()[2] > 0
    wired.close()
    orc.close()


# the table's vectors that go into the ticks: all but the 65,536-byte runs (the same path as the 800-byte run:
# more frames than an InputQueue holds; 65,536 frames of expectation per tick would only slow the test)
INJECTED = [r for r in TABLE if "65536" not in r[0]]
OVER_CAPACITY = {"zero_run_800-ib1", "zero_run_800-ib2", "zero_run_800-ib4"}  # 800 / 400 / 200 frames


@pytest.mark.gpu
@pytest.mark.parametrize("tpl", [1, 30], ids=["live", "fused"])
@pytest.mark.parametrize("ib", [1, 4], ids=["ex_game", "stub"])
def test_gpu_every_vector_inside_the_ticks(gpu_available, ib, tpl):
    """Every vector replaces the packet of one tick in a session of its own, in an otherwise healthy batch.
    A malformed or partial-input vector stops exactly its session (RB_PANIC, decode status -1); a valid
    one is decoded like the oracle decodes it and the session plays on with those inputs; the 800-byte
    zero run is valid and carries more frames than an InputQueue holds: InputQueue's length assert
    panics the session in the oracle and on the device.  Every other session plays on untouched."""
    import torch

    import ggrs_amd as G
    from ggrs_amd import _lib as L
    from ggrs_amd.p2p import synth_network
    from test_wire import _encode_schedule, _oracle_packet_deliveries
    lib = L.load()
    game, orc_game, dt, imask = ((G.Game.EX_GAME, O.EX_GAME, np.uint8, 0xFF) if ib == 1 else
                                 (G.Game.STUB, O.STUB, np.uint32, 0xFFFFFFFF))
    S, P, mask, rd, W, stride, T, bad_t = 200, 2, 0b01, 1, 8, 96, 60, 20
    rows = [r for r in INJECTED if r[1] == ib]
    where = {2 + 5 * i: r for i, r in enumerate(rows)}
    assert max(where) < S and max(len(r[3]) for r in rows) <= stride
    inputs, upto, rin = synth_network(S, P, T, mask, rd, 1, 4, dtype=dt, mask=imask)
    # the sender of a vector's session sends nothing new at bad_t (its place is the vector's), so its next
    # packet starts where the receiver stood before the vector and never skips a frame (no gap assert)
    sent = upto.copy()
    sent[bad_t, 1, list(where)] = upto[bad_t - 1, 1, list(where)]
    pk, ln, st = _encode_schedule(lib, P, S, T, mask, rd, sent, torch.from_numpy(rin).cuda(), stride, seed=30 + ib,
                                  ib=ib)
    for s_, (_, _, _, packet, _) in where.items():
        pk[bad_t, 1, s_, :] = 0
        pk[bad_t, 1, s_, :len(packet)] = torch.tensor(list(packet), dtype=torch.uint8)
        ln[bad_t, 1, s_] = len(packet)
        st[bad_t, 1, s_] = int(upto[bad_t - 1, 1, s_]) + 1  # the frame after the last one received
    F = int(st[bad_t, 1].max()) + 800 // ib + 8  # the restatement's recv_inputs: room for the longest vector
    assert F >= rin.shape[0]
    uptos, recvs, codes = _oracle_packet_deliveries(P, S, T, mask, W, F, pk, ln, st, ib=ib)
    assert (np.delete(codes, bad_t, axis=0) >= 0).all()  # every other packet of the schedule is one the reference accepts
    dead_at = {}
    for s_, (name, _, _, _, want) in where.items():
        assert (codes[bad_t, 1, s_] == -1) == (want is None), name
        if want is None:
            dead_at[s_] = bad_t
    assert len(dead_at) >= 8 and len(where) - len(dead_at) >= 8
    wired = _start(game, S, P, W, rd, mask)
    orc = O.OracleP2P(orc_game, P, W, 1, mask, S, sparse_saving=False, remote_delay=rd)
    chunks = (tpl,) * (T // tpl)
    alive = run_packets_against_oracle(wired, orc, P, mask, inputs, pk, ln, st, uptos, recvs, codes, chunks, dead_at)
    over = {s_ for s_, r in where.items() if r[0] in OVER_CAPACITY}
    assert len(over) == 1
    np.testing.assert_array_equal(np.nonzero(~alive)[0], sorted(set(dead_at) | over))
    wired.close()
    orc.close()
