"""The network-fed P2P kernels (the kP2PNet flag sets of ggrs_amd/csrc/p2p_variant.hpp) against the
oracle on every game and launch form.

Desync detection (desync_interval > 0) or the peers' connect-status reports select a family of
p2p_kernel instantiations of their own: cells and the input ring in HBM, the lead lane's snapshot of
the cells check_checksum_send_interval reads (p2p.hpp CellSnap), desync_step's histories, outbox and
event rings, the sparse path's unconditional dry run, the queue asserts folded into the status by
group_min<L>.  Here one GPU batch A runs against its oracle twin OA (O.OracleP2P, the same local
mask) while one oracle peer per remote handle of A produces the ChecksumReports A receives; every
comparison is exact equality, after every call of 1, 7 or 29 ticks:

  status, LoadGameState frame, AdvanceFrame and SaveGameState counts of the call's last tick;
  A.take_checksum_reports() against OA.take_checksum_reports(8);
  A.desync_events() against OA.desync_events(RB_P2P_EVENTS_KEPT), all five arrays;
  cells, live state, frames and queues (test_p2p.compare_state) after fused calls, every 10th
  one-tick call and the last call.

The oracle knows no fan-out: a fan-out batch must be observably the plain oracle.  The oracle side
of a (row, plan) runs once per process (oracle_trace) and is shared by the GPU test, the tick-log
twin and the CPU witness of that row.

Rows, and the flag set each launches (tests/check_net_variants.cpp prints them from p2p_choose; the
witness test asserts this table and that it covers every kP2PNet flag set p2p_variant_reachable
allows and some launch can choose):

  row     game       P, mask    path                               d/lag/interval  plans  flag set
  1       ex_game    2, 0b01    plain, W = 12                      2/(1,4)/5       7, 29  Net
  2       ex_game    3, 0b001   plain                              1/(1,4)/4       1, 7   Net
  3       ex_game    4, 0b0011  plain                              1/(1,4)/5       1, 29  Net
  4       ex_game    2, 0b01    fan-out K = 16, in-kernel          1/(1,5)/5       1, 29  Net|Spec
  5       ex_game    4, 0b0001  fan-out per player                 1/(1,5)/5       1, 29  Net|Spec
  6       ex_game    4, 0b0001  fan-out one player, K = 6          1/(1,5)/5       1, 7   Net|Spec|Mtf
  7       ex_game    2, 0b01    fan-out, RB_FANOUT_GENERIC=1       1/(1,5)/5       1      Net|Spec
  8       brawler    2, 0b01    plain                              1/(1,4)/5       1, 7   Net
  9       brawler    3, 0b010   plain, W = 6                       1/(1,4)/3       7      Net
  10      brawler    2, 0b01    fan-out K = 16, input mask 0x07    1/(1,5)/5       1, 7   Net|Spec|Mtf
  11      stub       2, 0b01    plain, u32 inputs (mask 0x3)       1/(1,4)/5       1, 29  Net
  12      stub_enum  2, 0b10    plain (mask 0x1)                   1/(1,4)/5       1      Net
  13b/13s brawler, stub 2, 0b01 sparse saving                      1/(1,3)/4       1      Net|Sparse
  14      ex_game, brawler 2, 0b01  plain, interval 1 / 3          1/(1,4)/1, 3    7 / 29 Net
  15      orbit      3, 0b001   plain, desync + peer status        1/(1,4)/5       1      Net
  peer-brawler-sp0/1  brawler   3, 0b001  peer status, sparse and not   1/(1,3)/0    1, 7 / 1  Net, Net|Sparse
  peer2-*-sp0/1  stub, stub_enum  2, 0b01  peer status, sparse and not  1/(1,3)/0    1, 7 / 1  Net, Net|Sparse
  peer-brawler-desync  brawler  3, 0b001  desync + peer status     1/(1,4)/5       1      Net
  4, 8, 10, 11 with the tick log (enable_time_sync)                                       ... |Log
  (ex_game's Net|Sparse: test_p2p_desync.py's sparse case and test_p2p_peer_status.py, not here)

Rows with peers' reports (15, peer-*) take test_p2p_peer_status.py's schedule, which disconnects a
player in sessions 0-15 and panics sessions 8-15 by design: their witness is that test's three class
conditions, and the conditions of the other rows hold over the sessions the schedule leaves alone
(16 and up).  The device's stub games take exactly two players, so that three-player schedule cannot
be created for them; the peer2-* rows run its two-player restatement (two_player_reports), in which
the disconnect is not re-triggered, with the witness that follows from that.
"""
import functools
import os
import subprocess
from collections import namedtuple

import numpy as np
import pytest

import ggrs_amd as G
from ggrs_amd._lib import RB_NULL_FRAME, RB_P2P_EVENTS_KEPT, RB_P2P_REPORTS_PER_TAKE, RB_PANIC
from ggrs_amd.p2p import PlayerType, synth_network
from ggrs_amd.synth import SEED
from oracle import oracle as O
from test_p2p import ORC_GAME, compare_state, drive_oracle
from test_p2p_desync import ORC_PANIC, dev_reports_as_oracle
from test_p2p_peer_status import drive as drive_peer_status
from test_p2p_peer_status import reports as peer_status_reports
from test_plugin_game import ORC as ORBIT_ORACLE
from test_plugin_game import PLUGIN as ORBIT_PLUGIN
from test_time_sync import FPS

_TESTS = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_TESTS), "ggrs_amd", "csrc")

PLAN_TICKS = {1: 90, 7: 91, 29: 116}
T_REP = 25  # the peers' connect-status reports are given before this tick (test_p2p_peer_status.py)
ORBIT = "orbit"  # the plug-in game of tests/plugin_game
# A persistent canonical state word per game, flipped by debug_corrupt / corrupt: a value the game adds
# to and never resets, so the offset stays (test_oracle_corruption_persists).  ex_game: player 0's rotation
# (word 4P, as test_p2p_desync.py); the brawler: the first AI entity's COUNTER (entity P, field 7);
# the stubs: their one state word; orbit: HITS (word 4 * 3 + 1).
CORRUPT_MASK = 0x00100000


def corrupt_word(game, P):
    return {G.Game.EX_GAME: 4 * P, G.Game.BRAWLER: P * 8 + 7, ORBIT: 13}.get(game, 0)


# fan: None, or (K candidates, per player, RB_FANOUT_GENERIC); peer: the peers' connect-status reports, 0 (off),
# 3 (test_p2p_peer_status.py's three-player schedule) or 2 (its two-player restatement, two_player_reports)
Row = namedtuple("Row", "key game P mask W d rd lag interval sparse fan imask S peer T plans")


def _row(key, game, P, mask, lag, interval, plans, W=8, d=1, rd=None, sparse=False, fan=None, imask=None, S=None,
         peer=0, T=None):
    if imask is None:
        imask = {G.Game.STUB: 0x3, G.Game.STUB_ENUM: 0x1, ORBIT: 0x1F}.get(game, 0x0F)
    if S is None:
        S = 10 if game == G.Game.BRAWLER else 70
    return Row(key, game, P, mask, W, d, d if rd is None else rd, lag, interval, sparse, fan, imask, S, peer, T,
               tuple(plans))


EX, BR, ST, SE = G.Game.EX_GAME, G.Game.BRAWLER, G.Game.STUB, G.Game.STUB_ENUM
ROWS = [
    _row("1", EX, 2, 0b01, (1, 4), 5, (7, 29), W=12, d=2),
    _row("2", EX, 3, 0b001, (1, 4), 4, (1, 7)),
    _row("3", EX, 4, 0b0011, (1, 4), 5, (1, 29)),
    _row("4", EX, 2, 0b01, (1, 5), 5, (1, 29), fan=(16, False, False)),
    _row("5", EX, 4, 0b0001, (1, 5), 5, (1, 29), fan=(16, True, False)),
    _row("6", EX, 4, 0b0001, (1, 5), 5, (1, 7), fan=(6, False, False)),
    _row("7", EX, 2, 0b01, (1, 5), 5, (1,), fan=(16, False, True)),
    _row("8", BR, 2, 0b01, (1, 4), 5, (1, 7)),
    _row("9", BR, 3, 0b010, (1, 4), 3, (7,), W=6),
    _row("10", BR, 2, 0b01, (1, 5), 5, (1, 7), fan=(16, False, False), imask=0x07),
    _row("11", ST, 2, 0b01, (1, 4), 5, (1, 29)),
    _row("12", SE, 2, 0b10, (1, 4), 5, (1,)),
    _row("13b", BR, 2, 0b01, (1, 3), 4, (1,), sparse=True),
    _row("13s", ST, 2, 0b01, (1, 3), 4, (1,), sparse=True),
    _row("14-ex-i1", EX, 2, 0b01, (1, 4), 1, (7,)),
    _row("14-ex-i3", EX, 2, 0b01, (1, 4), 3, (29,)),
    _row("14-br-i1", BR, 2, 0b01, (1, 4), 1, (7,)),
    _row("14-br-i3", BR, 2, 0b01, (1, 4), 3, (29,)),
    _row("15", ORBIT, 3, 0b001, (1, 4), 5, (1,), peer=3),
]
# section 3: test_p2p_peer_status.py's schedule (P = 3, handle 0 local, input delay 1, remote delay 2,
# lag 1-3, 60 ticks, reports before tick 25) beyond ex_game; the non-sparse rows also in 7-tick calls
PEER_ROWS = [_row(f"peer-brawler-sp{int(sp)}", BR, 3, 0b001, (1, 3), 0, (1,) if sp else (1, 7), rd=2, sparse=sp, S=32,
                  peer=3, T=60) for sp in (False, True)]
PEER_ROWS.append(_row("peer-brawler-desync", BR, 3, 0b001, (1, 4), 5, (1,), S=32, peer=3))
# The device's stub games take exactly two players (ops_stub.hip: the stubs sum two inputs, stubs.rs:114-118),
# so the three-player schedule cannot be built for them: rb_p2p_create refuses.  Their rows run its
# two-player restatement (two_player_reports): the one remote endpoint makes the same three reports.
PEER_ROWS += [_row(f"peer2-{g.name.lower()}-sp{int(sp)}", g, 2, 0b01, (1, 3), 0, (1,) if sp else (1, 7), rd=2, sparse=sp,
                   S=64, peer=2, T=60) for g in (ST, SE) for sp in (False, True)]
ALL_ROWS = {r.key: r for r in ROWS + PEER_ROWS}
CASES = [(r.key, n) for r in ROWS + PEER_ROWS for n in r.plans]
CASE_IDS = [f"row{k}-plan{n}" for k, n in CASES]
LOG_CASES = [(k, n) for k in ("4", "8", "10", "11") for n in ALL_ROWS[k].plans]  # section 4


def row_seed(row):
    return SEED + list(ALL_ROWS).index(row.key)  # one seed per row


def row_ticks(row, n):
    return row.T or PLAN_TICKS[n]


def plan_calls(T, n, cut=None):
    """Calls (t0, t1) of n ticks over [0, T), with a call boundary at `cut`."""
    edges = sorted(set(list(range(0, T, n)) + [T] + ([cut] if cut is not None else [])))
    return list(zip(edges[:-1], edges[1:]))


def corrupted_sessions(row):
    # the first, the last, and the first session of the partial last wave next to the pad columns
    return [0, 64 if row.S > 64 else row.S // 2, row.S - 1]


def is_corrupted(row):
    # Fan-out rows are not corrupted: rb_p2p_debug_corrupt flips the live state and the cells but not the
    # fan-out's branch planes, so the next select would undo the flip on the device only.  Their events
    # come from the lag: predicted frames get reported (the reference's false positives).  With sparse
    # saving every session panics within the first report or two; rows without desync detection have no
    # checksums to disagree.
    return row.fan is None and not row.sparse and row.interval > 0


def two_player_reports(S, upto, t, d):
    """test_p2p_peer_status.reports with one remote endpoint: before tick t endpoint 1 reports player 1
    (itself) disconnected at the frame we hold (sessions 0..7) or 2 frames before it (8..15), the local
    player 0 disconnected (16..23: a no-op), and plain connected statuses (24..).  With the endpoint
    gone after the disconnect nobody re-triggers it, so sessions 8..15 roll back once and go on."""
    held = upto[t]
    last = np.stack([np.full(S, t - 1 + d, np.int32), np.maximum(held[1], -1)]).astype(np.int32)
    disc = np.zeros((2, S), np.uint8)
    disc[1, 0:16] = 1
    last[1, 8:16] = held[1, 8:16] - 2
    disc[0, 16:24] = 1
    return [(1, last, disc)]


def oracle_tick(orc, mask, inputs, upto, rin, t):
    # (test_p2p.drive_oracle asserts that no delivery panics; with peers' reports one may)
    for h in range(inputs.shape[1]):
        if not (mask >> h) & 1:
            orc.deliver(h, upto[t, h], rin[:, h, :])
    for h in range(inputs.shape[1]):
        if (mask >> h) & 1:
            orc.add_local_input(h, inputs[t, h])
    return orc.advance()


def remote_handles(row):
    return [h for h in range(row.P) if not (row.mask >> h) & 1]


def oracle_reports_as_dev(frames, checksums):
    """ChecksumReports in the oracle's layout (frames [K, S] int32, checksums [K, S, 2] uint64 lo / hi)
    as the device's [K, S, 3] int64 rows: lo, hi, frame | RB_NULL_FRAME << 32 (no mismatch frame)."""
    frames = np.ascontiguousarray(frames, np.int32)
    cs = np.ascontiguousarray(checksums, np.uint64)
    out = np.empty(frames.shape + (3,), np.uint64)
    out[..., 0] = cs[..., 0]
    out[..., 1] = cs[..., 1]
    out[..., 2] = frames.view(np.uint32).astype(np.uint64) | (np.uint64(RB_NULL_FRAME & 0xFFFFFFFF) << np.uint64(32))
    return out.view(np.int64)


# ---------------------------------------------------------------------------- the oracle side, once
class Snapshot:
    """What compare_state reads of an oracle batch, kept."""

    def __init__(self, orc):
        self._cells, self._live, self._frames, self._queues = orc.read_cells(), orc.read_live(), orc.frames(), orc.queues()

    def read_cells(self):
        return self._cells

    def read_live(self):
        return self._live

    def frames(self):
        return self._frames

    def queues(self):
        return self._queues


Call = namedtuple("Call", "t0 t1 corrupt peer_status status reports peer_reports events alive state")
Trace = namedtuple("Trace", "row inputs upto rin calls cur st lf sent")


def make_oracle(row, mask, sparse=None):
    game = O.PLUGIN if row.game == ORBIT else ORC_GAME[row.game]
    kw = dict(lib_path=ORBIT_ORACLE) if row.game == ORBIT else {}
    orc = O.OracleP2P(game, row.P, row.W, row.d, mask, row.S, sparse_saving=row.sparse if sparse is None else sparse,
                      remote_delay=row.rd, **kw)
    if row.interval:
        orc.set_desync_detection(row.interval)
    return orc


def network(row, T, mask):
    dt = np.uint32 if row.game == ST else np.uint8
    return synth_network(row.S, row.P, T, mask, row.rd, row.lag[0], row.lag[1], seed=row_seed(row), dtype=dt,
                         mask=row.imask)


@functools.lru_cache(maxsize=None)
def oracle_trace(key, n):
    """Row `key` in calls of n ticks on the oracle alone: OA, its peers, and everything a GPU batch fed
    the same calls must reproduce."""
    row = ALL_ROWS[key]
    T = row_ticks(row, n)
    inputs, upto, rin = network(row, T, row.mask)
    oa = make_oracle(row, row.mask)
    peers = {}
    for h in remote_handles(row) if row.interval else []:
        pi, pu, pr = network(row, T, 1 << h)
        assert np.array_equal(pi, inputs) and np.array_equal(pr, rin)  # one set of inputs for every mask
        peers[h] = (make_oracle(row, 1 << h), pu)
    shadow = make_oracle(row, row.mask) if row.interval else None  # counts the reports a call sends (no take limit)
    sender = min(h for h in range(row.P) if (row.mask >> h) & 1)  # the handle A's reports arrive under at a peer
    calls = plan_calls(T, n, T_REP if row.peer else None)
    # the flip goes between the two calls nearest a third of the run
    t_bad = min((t0 for t0, _ in calls), key=lambda t0: abs(3 * t0 - T)) if is_corrupted(row) else None
    alive = np.ones(row.S, bool)
    cur, st_t, lf_t, sent, out = [], [], [], [], []

    def tick_oa(orc, t):
        if row.peer == 3:
            return drive_peer_status(orc, inputs, upto, rin, t)
        if row.peer == 2:
            return oracle_tick(orc, row.mask, inputs, upto, rin, t)
        return drive_oracle(orc, row.mask, inputs, upto, rin, t + 1, t0=t)[0]

    for i, (t0, t1) in enumerate(calls):
        bad = corrupted_sessions(row) if t0 == t_bad else []
        for s in bad:
            oa.corrupt(s, corrupt_word(row.game, row.P), CORRUPT_MASK)
        status_reports = []
        if row.peer and t0 == T_REP:
            status_reports = peer_status_reports(row.S, upto, t0) if row.peer == 3 else two_player_reports(row.S, upto, t0, row.d)
        for e, last, disc in status_reports:
            oa.receive_peer_connect_status(e, last, disc)
        for t in range(t0, t1):
            cur.append(oa.frames()[0])
            res = tick_oa(oa, t)
            st_t.append(res[0])
            lf_t.append(res[1])
            for h, (peer, pu) in peers.items():
                drive_oracle(peer, 1 << h, inputs, pu, rin, t + 1, t0=t)
            if shadow is not None:
                tick_oa(shadow, t)
        alive = alive & (res[0] != ORC_PANIC)
        rep = peer_reps = events = None
        if row.interval:
            rep = oa.take_checksum_reports(RB_P2P_REPORTS_PER_TAKE)
            peer_reps = {h: peer.take_checksum_reports(RB_P2P_REPORTS_PER_TAKE) for h, (peer, _) in peers.items()}
            for h, (f, c) in peer_reps.items():
                oa.receive_checksum_reports(h, f, c)
                peers[h][0].receive_checksum_reports(sender, *rep)
            events = oa.desync_events(RB_P2P_EVENTS_KEPT)
            sent.append((shadow.take_checksum_reports(64)[0] >= 0).sum(0))
        full = t1 - t0 > 1 or i % 10 == 9 or t1 == T or row.peer
        out.append(Call(t0, t1, bad, status_reports, res, rep, peer_reps, events, alive, Snapshot(oa) if full else None))
    return Trace(row, inputs, upto, rin, out, np.array(cur), np.array(st_t), np.array(lf_t), np.array(sent))


# ---------------------------------------------------------------------------- CPU: converter, corruption, witnesses
def test_oracle_reports_round_trip_through_the_device_layout():
    import torch
    K, S = RB_P2P_REPORTS_PER_TAKE, 5
    frames = np.full((K, S), RB_NULL_FRAME, np.int32)
    cs = np.zeros((K, S, 2), np.uint64)
    frames[0] = [9, 14, 0, 2**31 - 2, RB_NULL_FRAME]
    frames[1, :2] = [19, 24]
    cs[0, :, 0] = [1, 0x8000000000000000, 0xFFFFFFFFFFFFFFFF, 0x123456789ABCDEF0, 0]  # bit 63 set
    cs[0, :, 1] = [0, 0, 0x8000000000000001, 7, 0]
    cs[1, :2, 0] = [0xDEADBEEF00000000, 3]
    dev = oracle_reports_as_dev(frames, cs)
    assert dev.dtype == np.int64 and dev.shape == (K, S, 3)
    assert dev[0, 1, 0] == -2**63 and dev[0, 2, 0] == -1  # the same bits as int64
    assert (dev[..., 2] >> 32 == RB_NULL_FRAME).all()  # no mismatch frame
    assert (dev[frames == RB_NULL_FRAME][:, 2] == -1).all()  # a NULL_FRAME row: all ones
    assert dev[0, 0, 2] == 9 | (0xFFFFFFFF << 32) - 2**64
    f, c = dev_reports_as_oracle(torch.from_numpy(dev))
    np.testing.assert_array_equal(f, frames)
    np.testing.assert_array_equal(c, cs)


@pytest.mark.parametrize("key", ["1", "8", "11", "12", "15"])
def test_oracle_corruption_persists(key):
    # the word chosen for each game keeps its offset: after the rest of the run the corrupted sessions'
    # live states still differ from a clean run's, the other sessions' in nothing
    row = ALL_ROWS[key]
    T = 60
    inputs, upto, rin = network(row, T, row.mask)
    runs = []
    for corrupt in (False, True):
        orc = make_oracle(row, row.mask)
        for t in range(T):
            if corrupt and t == T // 3:
                for s in corrupted_sessions(row):
                    orc.corrupt(s, corrupt_word(row.game, row.P), CORRUPT_MASK)
            drive_oracle(orc, row.mask, inputs, upto, rin, t + 1, t0=t)
        runs.append(orc.read_live()[0])
    diff = (runs[0] != runs[1]).sum(1)
    bad = np.zeros(row.S, bool)
    bad[corrupted_sessions(row)] = True
    assert (diff[bad] > 0).all() and (diff[~bad] == 0).all(), diff


@pytest.mark.parametrize("key,n", CASES, ids=CASE_IDS)
def test_oracle_schedule_reaches_what_the_row_is_for(key, n):
    tr = oracle_trace(key, n)
    row, last = tr.row, tr.calls[-1]
    panicked = ~last.alive
    first_panic = np.where((tr.st == ORC_PANIC).any(0), (tr.st == ORC_PANIC).argmax(0), -1)
    kept = np.arange(row.S) >= 16 if row.peer else np.ones(row.S, bool)  # (the peers' reports panic sessions by design)
    if row.peer == 3:  # test_p2p_peer_status.py's three classes
        assert last.alive[:8].any() and not last.alive[8:16].any() and last.alive[16:].all()
        assert (first_panic[8:16] >= T_REP).all()
    if row.peer == 2:
        # the two-player restatement: the report disconnects player 1 in sessions 0..15 and rolls them back
        # in its tick; a disconnect at the current frame panics (sync_layer.rs:141-145), the others go on
        # with the player gone; sessions 16 and up never panic and keep it
        gone = last.state.queues()[:, 1, 7] == 1
        assert last.alive[:8].any() and last.alive[8:16].any() and last.alive[16:].all()
        assert gone[:16][last.alive[:16]].all() and not gone[16:].any()
        assert (first_panic[:16][~last.alive[:16]] >= T_REP).all()
        assert (tr.lf[T_REP, :16] != G.NULL_FRAME).any()
    if row.sparse and row.interval:
        # sparse saving with desync detection: frame last_saved - 1 has no cell (p2p_session.rs:907-910).
        # The test's value is the panic tick: a send needs current % interval == 0 and frame_to_send =
        # last_saved - 1 <= current - 1 above W, so no panic comes before such a tick.
        assert panicked.all()
        at = tr.cur[first_panic, np.arange(row.S)]
        assert (at % row.interval == 0).all() and (at - 1 > row.W).all(), at
        return
    if not row.interval:
        return
    assert not panicked[kept].any()
    taken = np.array([(c.reports[0] >= 0).sum(0) for c in tr.calls])  # [calls, S] reports per take
    assert (taken.sum(0) > 0)[kept].all()  # every session sends reports
    counts = last.events[0]
    assert (counts[kept] > 0).sum() * 3 >= kept.sum(), counts  # at least a third hold events
    # a tick that sends (current % interval == 0) and rolls back: the one CellSnap is there for
    assert ((tr.cur % row.interval == 0) & (tr.lf != G.NULL_FRAME) & (tr.st == 0)).any()
    if is_corrupted(row):
        assert any(c.corrupt for c in tr.calls)
        assert (counts[[s for s in corrupted_sessions(row) if kept[s]]] > 0).all(), counts
    if key.startswith("14") and row.interval == 1:
        assert (taken == 7).any()  # a report every tick: 7 per take
    if key.startswith("14") and row.interval == 3:
        # more reports in a launch than the outbox holds: the take has the newest 8
        assert (tr.sent > RB_P2P_REPORTS_PER_TAKE).any() and (taken == RB_P2P_REPORTS_PER_TAKE).any()
        over = tr.sent > RB_P2P_REPORTS_PER_TAKE
        assert (taken[over] == RB_P2P_REPORTS_PER_TAKE).all()


# ---------------------------------------------------------------------------- CPU: the flag sets the rows launch
# check_net_variants.cpp's trait sets.  ex_game with three players pads to four lanes; orbit, like the
# stubs, has one lane per session and no fan-out, and the rule reads nothing else of a game once kNet is set.
GROUP = {EX: "ex", BR: "brawler", ST: "stub", SE: "stub", ORBIT: "stub"}


def traits(row):
    return ("ex2" if row.P == 2 else "ex4") if row.game == EX else GROUP[row.game]


LAUNCHED = {  # the docstring's table
    "1": "Net", "2": "Net", "3": "Net", "4": "Net|Spec", "5": "Net|Spec", "6": "Net|Spec|Mtf", "7": "Net|Spec",
    "8": "Net", "9": "Net", "10": "Net|Spec|Mtf", "11": "Net", "12": "Net", "13b": "Net|Sparse", "13s": "Net|Sparse",
    "14-ex-i1": "Net", "14-ex-i3": "Net", "14-br-i1": "Net", "14-br-i3": "Net", "15": "Net",
    "peer-brawler-sp0": "Net", "peer-brawler-sp1": "Net|Sparse", "peer2-stub-sp0": "Net", "peer2-stub-sp1": "Net|Sparse",
    "peer2-stub_enum-sp0": "Net", "peer2-stub_enum-sp1": "Net|Sparse", "peer-brawler-desync": "Net",
}
# every kP2PNet flag set p2p_variant_reachable allows and some launch can choose, per trait set
WANTED = {
    "ex": {"Net", "Net|Sparse", "Net|Spec", "Net|Spec|Mtf", "Net|Spec|Log"},
    "brawler": {"Net", "Net|Sparse", "Net|Spec|Mtf", "Net|Log", "Net|Spec|Mtf|Log"},
    "stub": {"Net", "Net|Sparse", "Net|Log"},
}
ELSEWHERE = {("ex", "Net|Sparse")}  # test_p2p_desync.py (sparse case), test_p2p_peer_status.py (sparse)


def _facts(row, n, log):
    """check_net_variants' arguments: one launch for every call length of the plan."""
    T = row_ticks(row, n)
    lengths = sorted({t1 - t0 for t0, t1 in plan_calls(T, n, T_REP if row.peer else None)})
    K, _, generic = row.fan or (16, False, False)
    if generic:
        lengths = [1]  # fanout_kernel between the ticks: one-tick launches (rb_p2p_run_ticks)
    return [f"{traits(row)}:{t}:{row.W}:{int(row.sparse)}:{int(row.fan is not None)}:{int(generic)}:{K}:"
            f"{int(log)}:{int(row.interval > 0)}:{int(row.peer > 0)}" for t in lengths]


def test_rows_launch_every_reachable_net_flag_set(tmp_path):
    exe = str(tmp_path / "check_net_variants")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", _CSRC, "-o", exe,
                    os.path.join(_TESTS, "check_net_variants.cpp")], check=True)
    jobs = [(key, n, False) for key, n in CASES] + [(key, n, True) for key, n in LOG_CASES]
    args, owner = [], []
    for key, n, log in jobs:
        for a in _facts(ALL_ROWS[key], n, log):
            args.append(a)
            owner.append((key, log))
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    sets = {"reachable": {}, "choosable": {}, "chosen": []}
    for line in r.stdout.splitlines():
        kind, *rest = line.split()
        if kind == "chosen":
            sets[kind].append(rest[0])
        else:
            sets[kind][rest[0]] = set(rest[1:])
    assert len(sets["chosen"]) == len(args)
    got = {}
    for (key, log), flags in zip(owner, sets["chosen"]):
        assert flags == LAUNCHED[key] + ("|Log" if log else ""), (key, log, flags)  # the table: one flag set per row
        got.setdefault(GROUP[ALL_ROWS[key].game], set()).add(flags)
    for name, want in WANTED.items():
        for t in ("ex2", "ex4") if name == "ex" else (name,):
            # the rule can choose exactly the flag sets wanted here, each with and without the tick log
            # (section 4 has rows for some of those with it), and the game instantiates them all
            plain = {f for f in want if "Log" not in f}
            assert sets["choosable"][t] == plain | {f + "|Log" for f in plain}, (t, sets["choosable"][t])
            assert sets["choosable"][t] <= sets["reachable"][t]
        missing = want - got[name] - {f for g, f in ELSEWHERE if g == name}
        assert not missing, (name, missing)  # ... and some row launches every one of them
        assert not {f for g, f in ELSEWHERE if g == name} & got[name]


# ---------------------------------------------------------------------------- GPU
def gpu_batch(row, time_sync=False):
    from ggrs_amd.plugin import register_game_plugin
    game = register_game_plugin(ORBIT_PLUGIN) if row.game == ORBIT else row.game
    b = (G.SessionBuilder(game, num_sessions=row.S).with_num_players(row.P).with_max_prediction_window(row.W)
         .with_input_delay(row.d).with_remote_input_delay(row.rd).with_sparse_saving_mode(row.sparse)
         .with_desync_detection_mode(row.interval).with_peer_connect_status(row.peer > 0))
    if row.fan:  # always on: every launch of the row takes the fan-out's flag set
        b.with_speculative_fanout(True, row.fan[0], adaptive=False, per_player=row.fan[1])
    for h in range(row.P):
        b.add_player(PlayerType.Local if (row.mask >> h) & 1 else PlayerType.Remote, h)
    sess = b.start_p2p_session()
    if time_sync:
        sess.enable_time_sync(FPS)
    return sess


EVENT_ARRAYS = ("counts", "frames", "handles", "local", "remote")


def replay(tr, monkeypatch, twin=False):
    """The trace's calls on a GPU batch A: everything the oracle recorded, compared after every call.
    twin: a second batch with the tick log on (enable_time_sync) takes the same calls and received
    reports and must equal A in everything after every call."""
    import torch
    row = tr.row
    monkeypatch.setenv("RB_FANOUT_GENERIC", "1" if row.fan and row.fan[2] else "0")
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    di, du, dr = dev(tr.inputs), dev(tr.upto), dev(tr.rin)
    batches = [gpu_batch(row)] + ([gpu_batch(row, time_sync=True)] if twin else [])
    a = batches[0]
    alive = np.ones(row.S, bool)
    for c in tr.calls:
        what = f"row {row.key}, ticks [{c.t0}, {c.t1})"
        for g in batches:
            for s in c.corrupt:
                g.debug_corrupt(s, corrupt_word(row.game, row.P), CORRUPT_MASK)
            for e, last, disc in c.peer_status:
                g.receive_peer_connect_status(e, dev(last), dev(disc))
            g.run_ticks(di[c.t0:c.t1], du[c.t0:c.t1], dr)
        ost, olf, ona, ons = c.status
        st, lf, na, ns = a.status()
        np.testing.assert_array_equal(st[alive], np.where(ost == ORC_PANIC, RB_PANIC, ost)[alive], err_msg=f"status, {what}")
        alive = c.alive  # a panicked session is dead: compared no further
        np.testing.assert_array_equal(lf[alive], olf[alive], err_msg=f"LoadGameState frame, {what}")
        np.testing.assert_array_equal(na[alive], ona[alive], err_msg=f"AdvanceFrame count, {what}")
        np.testing.assert_array_equal(ns[alive], ons[alive], err_msg=f"SaveGameState count, {what}")
        reps = []
        if row.interval:
            reps = [g.take_checksum_reports() for g in batches]
            gf, gc = dev_reports_as_oracle(reps[0])
            of, oc = c.reports
            np.testing.assert_array_equal(gf[:, alive], of[:, alive], err_msg=f"report frames, {what}")
            has = (of >= 0) & alive[None, :]
            np.testing.assert_array_equal(gc[has], oc[has], err_msg=f"report checksums, {what}")
            for h, (f, cs) in c.peer_reports.items():
                peer = dev(oracle_reports_as_dev(f, cs))
                for g in batches:
                    g.receive_checksum_reports(h, peer)
            for x, y, name in zip(a.desync_events(), c.events, EVENT_ARRAYS):
                np.testing.assert_array_equal(x[alive], y[alive], err_msg=f"desync events {name}, {what}")
        if c.state is not None:  # (rows with peers' reports: after every call, the queues among it)
            compare_state(a, c.state, c.t1 - 1, alive)
        if twin:
            b = batches[1]
            for x, y, name in zip(b.status(), (st, lf, na, ns), ("status", "load frame", "AdvanceFrames", "saves")):
                np.testing.assert_array_equal(x, y, err_msg=f"tick-log twin {name}, {what}")
            assert torch.equal(reps[1], reps[0]), f"tick-log twin reports, {what}"
            for x, y, name in zip(b.desync_events(), a.desync_events(), EVENT_ARRAYS):
                np.testing.assert_array_equal(x, y, err_msg=f"tick-log twin events {name}, {what}")
            for x, y in zip(b.read_cells() + (b.read_live(), b.read_queues()) + b.frames(),
                            a.read_cells() + (a.read_live(), a.read_queues()) + a.frames()):
                np.testing.assert_array_equal(x, y, err_msg=f"tick-log twin cells, live state, queues or frames, {what}")
    if row.fan:
        adv, saves, loads, selects, branch_frames = a.totals()
        assert selects > 0, "no misprediction was served by a branch select"
        assert branch_frames > 0
        assert a.counters()[1] == 0  # no lane took the out-of-range math path: no select handed a lane garbage
    assert a.counters()[2] == (~alive).sum()  # each panicked session counted once
    for g in batches:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("key,n", CASES, ids=CASE_IDS)
def test_gpu_net_kernels_match_the_oracle(gpu_available, monkeypatch, key, n):
    replay(oracle_trace(key, n), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("key,n", LOG_CASES, ids=[f"row{k}-plan{n}" for k, n in LOG_CASES])
def test_gpu_tick_log_changes_nothing(gpu_available, monkeypatch, key, n):
    # kNet | kLog: the launches that also write the tick log compute what the ones without it do,
    # which in turn equals the oracle
    replay(oracle_trace(key, n), monkeypatch, twin=True)
