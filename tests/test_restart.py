"""Restarting single sessions of a P2P or spectator batch in place (include/ggrs_amd.h
rb_p2p_restart_sessions, rb_spectator_restart_sessions): dropping a
P2PSession and calling SessionBuilder::start_p2p_session (builder.rs:251-308) again with the same
builder, for the selected sessions only.

"Fresh" is defined by comparison, never by a list of values: a restarted session is compared with
an oracle session created at that moment, or with a batch created at that moment.

The cohort tests: session s is in cohort s % 3.  Cohort 0 is never restarted, cohort 1 once (after
37 ticks), cohort 2 twice (after 37 and after 90 ticks).  Every match of a cohort has a seeded
network of its own (lags 1-4, one stall longer than the prediction window); for tick t the batch's
local inputs, delivery watermarks and the columns of the remote inputs by frame come from the match
each session is in, at that match's own tick.  Every comparison is equality.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import ggrs_amd as G
from ggrs_amd import _lib as L
from ggrs_amd.p2p import PlayerType, synth_network
from ggrs_amd.synth import SEED
from oracle import oracle as O
from test_p2p import ORC_GAME
from test_p2p_pacing import Classes, compare_all, dev, everything, session_mask, snapshot
from test_time_sync import PEER, gpu_state, make_session, peer_reports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 8
S, T = 70, 130          # 70 sessions: two waves, one partial
RESTARTS = {37: (1, 2), 90: (2,)}   # before tick t (after t ticks): the cohorts restarted
NC = 3
STALL = (12, 23)        # of every match, in the sessions s % 5 == 1: 11 ticks > W


def cohort_of(n):
    return np.arange(n) % NC


def match_start(c, t):
    """The tick at which the match cohort c plays at tick t began."""
    return max([0] + [r for r, who in RESTARTS.items() if c in who and r <= t])


def match_network(P, mask, rd, n, c, start, ticks, dtype, imask):
    """The network of the match of cohort c that begins at tick `start` (all n columns; the cohort
    uses its own)."""
    seed = SEED ^ (0x51 + 0x1000 * (c + 1) + 0x10 * start)
    inputs, upto, rin = synth_network(n, P, ticks, mask, rd, 1, 4, seed=seed, dtype=dtype, mask=imask)
    h = [x for x in range(P) if not (mask >> x) & 1][0]
    who = np.arange(n) % 5 == 1
    upto[STALL[0]:STALL[1], h, who] = upto[STALL[0] - 1, h, who]
    return inputs, upto, rin


@functools.lru_cache(maxsize=None)
def assembled(P, mask, rd, n=S, ticks=T, dtype=np.uint8, imask=0x0F):
    """(local inputs [ticks, P, n], remote_upto [ticks, P, n], {phase start: remote inputs by frame
    [ticks + rd, P, n]}, {(cohort, match start): that match's network}): what the batch is handed."""
    co = cohort_of(n)
    starts = [0] + sorted(RESTARTS)
    nets = {(c, m): match_network(P, mask, rd, n, c, m, ticks, dtype, imask)
            for c in range(NC) for m in sorted({match_start(c, t) for t in starts})}
    inputs = np.zeros((ticks, P, n), dtype)
    upto = np.zeros((ticks, P, n), np.int32)
    for t in range(ticks):
        for c in range(NC):
            m = match_start(c, t)
            inputs[t][:, co == c] = nets[c, m][0][t - m][:, co == c]
            upto[t][:, co == c] = nets[c, m][1][t - m][:, co == c]
    phases = {}
    for p0 in starts:
        rin = np.zeros((ticks + rd, P, n), dtype)
        for c in range(NC):
            rin[:, :, co == c] = nets[c, match_start(c, p0)][2][:, :, co == c]
        phases[p0] = rin
    for a in (inputs, upto, *phases.values()):
        a.setflags(write=False)
    return inputs, upto, phases, nets


def phase_of(t):
    return max(p for p in [0] + sorted(RESTARTS) if p <= t)


class Cohorts(Classes):
    """test_p2p_pacing.Classes with one oracle per cohort that can be closed and made again."""

    def __init__(self, game, P, d, rd, mask, n, sparse=False, desync=0, lib_path=None):
        kw = {} if lib_path is None else {"lib_path": lib_path}
        orc_game = O.PLUGIN if lib_path else ORC_GAME[game]
        self._make = lambda k: O.OracleP2P(orc_game, P, W, d, mask, k, sparse_saving=sparse, remote_delay=rd, **kw)
        self.P, self.mask, self.n = P, mask, n
        self.cols = [np.arange(c, n, NC) for c in range(NC)]
        self.orcs = [self._make(len(k)) for k in self.cols]
        self.st = np.zeros(n, np.int32)
        self.lf, self.na, self.ns = (np.full(n, -1, np.int32) for _ in range(3))
        self.dead = np.zeros(n, bool)
        self.poll_panics = 0
        self._rin = (None, {})

    def restart(self, cohorts):
        for c in cohorts:
            k = self.cols[c]
            self.orcs[c].close()
            self.orcs[c] = self._make(len(k))
            self.st[k] = 0
            self.lf[k] = self.na[k] = self.ns[k] = -1
            self.dead[k] = False
        self._rin = (None, {})


ALL = np.ones(NC, bool)


def cohort_mask(n, cohorts):
    return np.isin(cohort_of(n), cohorts).astype(np.uint8)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_header_declares_and_library_exports_both_entry_points():
    header = open(os.path.join(ROOT, "include", "ggrs_amd.h")).read()
    assert re.search(r"rb_status rb_p2p_restart_sessions\(rb_p2p\* b, const uint8_t\* session_mask\);", header)
    assert re.search(r"rb_status rb_spectator_restart_sessions\(rb_spectator\* b, const uint8_t\* session_mask\);", header)
    lib = L.load()
    sig = {name: (res, args) for name, res, args in L.SIGNATURES}
    for name in ("rb_p2p_restart_sessions", "rb_spectator_restart_sessions"):
        assert sig[name] == (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p])
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int32 and fn.argtypes == [ctypes.c_void_p, ctypes.c_void_p]
    assert hasattr(G.P2PSession, "restart_sessions") and hasattr(G.SpectatorSession, "restart_sessions")


def test_cohort_assembly_feeds_every_match_its_own_network():
    """One plain OracleP2P per match, fed that match's own network directly, ends every tick where the
    cohort oracle fed from the assembled tensors does: the assembly hands match k of cohort c exactly
    its own columns at its own ticks."""
    P, mask, d, rd = 2, 0b01, 1, 1
    inputs, upto, phases, nets = assembled(P, mask, rd)
    co = cohort_of(S)
    cls = Cohorts(G.Game.EX_GAME, P, d, rd, mask, S)
    plain = {}
    saw_threshold = np.zeros(S, bool)
    for t in range(T):
        if t in RESTARTS:
            cls.restart(RESTARTS[t])
        for c in range(NC):
            m = match_start(c, t)
            k = cls.cols[c]
            if m == t:  # a new match: a new session
                if c in plain:
                    plain[c].close()
                plain[c] = O.OracleP2P(O.EX_GAME, P, W, d, mask, len(k), remote_delay=rd)
            li, up, rin = nets[c, m]
            np.testing.assert_array_equal(inputs[t][:, k], li[t - m][:, k])
            np.testing.assert_array_equal(upto[t][:, k], up[t - m][:, k])
            np.testing.assert_array_equal(phases[phase_of(t)][:, :, k], rin[:, :, k])
            assert plain[c].deliver(1, np.ascontiguousarray(up[t - m, 1][k]), np.ascontiguousarray(rin[:, 1][:, k])) == 0
            plain[c].add_local_input(0, np.ascontiguousarray(li[t - m, 0][k]))
            st = plain[c].advance()[0]
            saw_threshold[k] |= st == 1
        cls.tick(t, ALL, inputs, upto, phases[phase_of(t)])
        for c in range(NC):
            k = cls.cols[c]
            np.testing.assert_array_equal(plain[c].frames()[0], cls.frames()[0][k], err_msg=f"tick {t}")
            np.testing.assert_array_equal(plain[c].read_live()[0], cls.live()[k], err_msg=f"tick {t}")
    assert not cls.dead.any()
    assert saw_threshold[np.arange(S) % 5 == 1].all(), "every cohort has a stall longer than the window"
    want = np.array([T - match_start(c, T) for c in co])
    assert (cls.frames()[0] <= want).all() and (cls.frames()[0] > want - 16).all()
    for o in plain.values():
        o.close()
    cls.close()


# ---------------------------------------------------------------------------
# GPU 1: oracle parity, every tick
# ---------------------------------------------------------------------------
def orbit():
    from ggrs_amd.plugin import register_game_plugin
    from test_plugin_game import ORC, PLUGIN
    return register_game_plugin(PLUGIN), ORC


PARITY = {  # game, P, local mask, input delay, remote delay, sparse, sessions
    "stub-h0-d0": (G.Game.STUB, 2, 0b01, 0, 0, False, S),
    "stub-h1-d2-sparse": (G.Game.STUB, 2, 0b10, 2, 1, True, S),
    "exgame-p2-h0-d0": (G.Game.EX_GAME, 2, 0b01, 0, 0, False, S),
    "exgame-p2-h1-d2-sparse": (G.Game.EX_GAME, 2, 0b10, 2, 1, True, S),
    "exgame-p3-h1-d0-sparse": (G.Game.EX_GAME, 3, 0b010, 0, 1, True, S),
    "exgame-p3-h0-d2": (G.Game.EX_GAME, 3, 0b001, 2, 0, False, S),
    "exgame-p4-h0-d2": (G.Game.EX_GAME, 4, 0b0001, 2, 1, False, S),
    "exgame-p4-h1-d0-sparse": (G.Game.EX_GAME, 4, 0b0010, 0, 0, True, S),
    "brawler-h0-d2": (G.Game.BRAWLER, 2, 0b01, 2, 1, False, 6),
    "brawler-h1-d0-sparse": (G.Game.BRAWLER, 2, 0b10, 0, 0, True, 6),
    "orbit-h0-d1": ("orbit", 3, 0b001, 1, 2, False, S),
    "orbit-h1-d0-sparse": ("orbit", 3, 0b010, 0, 1, True, S),
}


def start(game, P, mask, d, rd, sparse, n, **kw):
    if game == "orbit":
        game = orbit()[0]
    return make_session(game, P, mask, d, rd, sparse=sparse, sessions=n, time_sync=kw.pop("time_sync", False), **kw)


def net_kind(game):
    return (np.uint32, 0x3) if game == G.Game.STUB else (np.uint8, 0x1F if game == "orbit" else 0x0F)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(PARITY))
def test_gpu_cohort_restarts_match_the_cohort_oracles_every_tick(gpu_available, case):
    game, P, mask, d, rd, sparse, n = PARITY[case]
    dtype, imask = net_kind(game)
    inputs, upto, phases, _ = assembled(P, mask, rd, n, T, dtype, imask)
    sess = start(game, P, mask, d, rd, sparse, n)
    cls = Cohorts(game, P, d, rd, mask, n, sparse=sparse, lib_path=orbit()[1] if game == "orbit" else None)
    di, du = dev(inputs, upto)
    dr = {p: dev(r) for p, r in phases.items()}
    saw_load = saw_threshold = False
    for t in range(T):
        if t in RESTARTS:
            sess.restart_sessions(cohort_mask(n, RESTARTS[t]))
            cls.restart(RESTARTS[t])
            compare_all(sess, cls, f"{case}, restart before tick {t}")
            sel = cohort_mask(n, RESTARTS[t]) != 0
            assert (sess.read_cells()[0][:, sel] == -1).all() and (sess.frames()[0][sel] == 0).all()
        sess.run_ticks(di[t:t + 1], du[t:t + 1], dr[phase_of(t)])
        cls.tick(t, ALL, inputs, upto, phases[phase_of(t)])
        compare_all(sess, cls, f"{case}, tick {t}")
        saw_load |= bool((cls.lf >= 0).any())
        saw_threshold |= bool((cls.st == 1).any())
    assert saw_load and saw_threshold and not cls.dead.any() and sess.counters()[2] == 0
    cur = sess.frames()[0]
    assert cur[0::3].min() > cur[1::3].max() and cur[1::3].min() > cur[2::3].max(), "the cohorts sit matches apart"
    sess.close()
    cls.close()


# ---------------------------------------------------------------------------
# GPU 2, 3: a fresh twin, with every hidden word dirtied first; neighbours untouched
# ---------------------------------------------------------------------------
DIRTY = dict(desync=10, peer=True, **PEER)   # ex_game P = 3, handle 0 local, D = 1, RD = 2
MATCH = 60
T_DISC, T_PEER, DIRTY_STALL = 15, 25, (30, 41)


@functools.lru_cache(maxsize=None)
def dirty_network(match):
    P, mask, rd = DIRTY["P"], DIRTY["mask"], DIRTY["RD"]
    inputs, upto, rin = synth_network(S, P, MATCH + 12, mask, rd, 1, 4, seed=SEED ^ (0xD1 + match))
    who = np.arange(S) % 5 == 1
    upto[DIRTY_STALL[0]:DIRTY_STALL[1], 1, who] = upto[DIRTY_STALL[0] - 1, 1, who]
    return inputs, upto, rin


def start_dirty():
    return make_session(G.Game.EX_GAME, DIRTY["P"], DIRTY["mask"], DIRTY["D"], DIRTY["RD"], desync=10, peer=True)


class Dirty:
    """One batch of the full configuration with the caller's tensors it owns: the pacer's mask, the
    spectators' feed."""

    def __init__(self, sess):
        import torch
        from test_spectator import Feed
        self.sess = sess
        self.run = torch.ones(S, dtype=torch.uint8, device="cuda")
        self.feed = Feed(sess, MATCH + 32)
        self.reports = None

    def readbacks(self):
        s = self.sess
        out = everything(s, True)
        del out["totals"], out["counters"]  # batch-wide: they continue since create
        out.update(zip(("ds_n", "ds_frame", "ds_handle", "ds_local", "ds_remote"), s.desync_events()))
        out.update(zip(("exp_status", "exp_next"), s.export_status()))
        out["parked"] = s.parked_ticks()
        out["run_mask"] = self.run.cpu().numpy()
        out["feed_inputs"], out["feed_upto"] = self.feed.inputs.cpu().numpy(), self.feed.upto.cpu().numpy()
        out["feed_last"], out["feed_disc"] = self.feed.last.cpu().numpy(), self.feed.disc.cpu().numpy()
        if self.reports is not None:
            out["reports"] = self.reports.cpu().numpy()
        return out


def session_axis(key, a):
    """The axis of read-back `key` that is the session."""
    if key in ("tags", "imgs", "cs", "reports"):
        return 1
    if key in ("local_adv", "remote_adv", "rtt", "windows", "feed_inputs", "feed_last", "feed_disc"):
        return a.ndim - 1
    return 0


def assert_equal_on(got, want, rows, what):
    assert got.keys() == want.keys()
    for k in want:
        ax = session_axis(k, want[k])
        np.testing.assert_array_equal(np.compress(rows, got[k], ax), np.compress(rows, want[k], ax), err_msg=f"{k}, {what}")


def drive_dirty(batches, match, t0, t1, rows=None, what=""):
    """Ticks [t0, t1) of match `match` on every batch in lock step: quality reports every 12 ticks
    (odd sessions ahead: they park), one disconnect_player, the peers' early-frame connect-status
    reports of test_time_sync.py (some sessions panic), a stall longer than the window, paced ticks
    with the masks rb_p2p_pace wrote, an export and an exchange of checksum reports (a few flipped)
    after every tick.  With rows: after every tick every read-back of batches[1:] equals
    batches[0]'s on those sessions."""
    P, mask, D = DIRTY["P"], DIRTY["mask"], DIRTY["D"]
    inputs, upto, rin = dirty_network(match)
    di, du, dr = dev(inputs, upto, rin)
    bad = dev(np.arange(S) % 7 == 3)
    for t in range(t0, t1):
        if t % 12 == 0:
            rtt = dev(np.full(S, 40 + 8 * (t // 12 % 3), np.int32))
            adv = dev(np.where(np.arange(S) % 2 == 1, 12 + t // 12 % 2, -3).astype(np.int32))
            for b in batches:
                for h in (1, 2):
                    b.sess.receive_quality(h, rtt, adv)
        if t == T_DISC:
            for b in batches:
                b.sess.disconnect_player(2, np.arange(S) % 7 == 5)
        if t == T_PEER:
            for e, last, disc in peer_reports(T_PEER, upto, P, D):
                for b in batches:
                    b.sess.receive_peer_connect_status(e, *dev(last, disc))
        for b in batches:
            s = b.sess
            s.advance_frame(di[t], du[t], dr, run=b.run)
            s.export_confirmed_inputs(b.feed.inputs, b.feed.upto, b.feed.last, b.feed.disc)
            b.reports = s.take_checksum_reports()
            echo = b.reports.clone()
            if t >= 20:
                echo[:, bad, 0] ^= 1
            s.receive_checksum_reports(1, echo)
            s.pace(out=b.run)
        if rows is not None:
            want = batches[0].readbacks()
            for i, b in enumerate(batches[1:]):
                assert_equal_on(b.readbacks(), want, rows, f"{what} batch {i + 1}, match {match} tick {t}")


def assert_dirtied(b):
    r = b.readbacks()
    assert (r["st"] == L.RB_PANIC).any() and (r["ds_n"] > 0).any() and (r["parked"] > 0).any()
    assert (r["counts"] > 0).any() or (r["frames_ahead"] != 0).any()
    assert (r["windows"] != 0).any() and (r["queues"][:, 2, 7] == 1).any() and (r["exp_next"] > 0).any()


@pytest.mark.gpu
def test_gpu_restart_all_equals_a_fresh_twin_with_every_feature_on(gpu_available):
    a = Dirty(start_dirty())
    drive_dirty([a], 0, 0, MATCH)
    assert_dirtied(a)
    panics = a.sess.counters()[2]
    a.sess.restart_sessions(None)
    assert a.sess.counters()[2] == panics > 0
    a, b = Dirty(a.sess), Dirty(start_dirty())  # the caller's tensors start again with the match
    everyone = np.ones(S, bool)
    assert_equal_on(b.readbacks(), a.readbacks(), everyone, "after the restart")
    drive_dirty([a, b], 1, 0, MATCH, rows=everyone, what="fresh twin")
    assert_dirtied(b)
    a.sess.close()
    b.sess.close()


@pytest.mark.gpu
@pytest.mark.parametrize("per_player", [True, False], ids=["per_player", "one_player"])
def test_gpu_restart_all_equals_a_fresh_fanout_twin(gpu_available, per_player):
    P, mask, d, rd = 2, 0b01, 0, 1

    def fan():
        b = (G.SessionBuilder(G.Game.EX_GAME, num_sessions=S).with_num_players(P).with_max_prediction_window(W)
             .with_input_delay(d).with_remote_input_delay(rd)
             .with_speculative_fanout(True, adaptive=False, per_player=per_player))
        for h in range(P):
            b.add_player(PlayerType.Local if (mask >> h) & 1 else PlayerType.Remote, h)
        return b.start_p2p_session()

    nets = [synth_network(S, P, MATCH, mask, rd, 1, 4, seed=SEED ^ (0xFA + m)) for m in range(2)]
    a = fan()
    di, du, dr = dev(*nets[0])
    for t in range(MATCH):
        a.run_ticks(di[t:t + 1], du[t:t + 1], dr)
    base = np.array(a.totals(), np.int64)
    assert base[3] > 0, "the first match must have selected branches"
    a.restart_sessions(None)
    b = fan()
    di, du, dr = dev(*nets[1])
    for t in range(MATCH):
        for x in (a, b):
            x.run_ticks(di[t:t + 1], du[t:t + 1], dr)
        want, got = everything(b, False), everything(a, False)
        for k in want:
            if k not in ("totals", "counters"):
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k}, tick {t}")
        np.testing.assert_array_equal(np.array(a.totals(), np.int64) - base, np.array(b.totals(), np.int64),
                                      err_msg=f"totals since the restart, tick {t}")
    assert b.totals()[3] > 0 and b.totals()[2] > 0
    a.close()
    b.close()


@pytest.mark.gpu
def test_gpu_restart_leaves_the_neighbours_bit_identical(gpu_available):
    a, twin, fresh = Dirty(start_dirty()), Dirty(start_dirty()), Dirty(start_dirty())
    drive_dirty([a, twin], 0, 0, MATCH - 10)
    assert_dirtied(a)
    sel = cohort_of(S) == 1
    before = a.readbacks()
    totals, counters = a.sess.totals(), a.sess.counters()
    a.sess.restart_sessions(sel)
    after = a.readbacks()
    assert_equal_on(after, before, ~sel, "cohorts 0 and 2 across the call")
    assert a.sess.totals() == totals and a.sess.counters() == counters
    for k in ("feed_inputs", "feed_upto", "feed_last", "feed_disc", "run_mask", "reports"):  # the caller's own tensors
        del after[k]
    want = fresh.readbacks()
    assert_equal_on(after, {k: want[k] for k in after}, sel, "cohort 1 against a batch just created")
    # the unrestarted twin and the batch go on together: nothing of cohort 1's restart leaks later either
    drive_dirty([twin, a], 0, MATCH - 10, MATCH, rows=~sel, what="neighbours")
    for b in (a, twin, fresh):
        b.sess.close()


# ---------------------------------------------------------------------------
# GPU 4: launch shapes with sessions hundreds of frames apart
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["exgame-p2", "exgame-p2-sparse", "brawler", "brawler-sparse"])
def test_gpu_launch_shapes_after_cohort_restarts(gpu_available, case):
    game, n = (G.Game.BRAWLER, 6) if case.startswith("brawler") else (G.Game.EX_GAME, S)
    sparse = case.endswith("sparse")
    P, mask, d, rd, ticks, t_split = 2, 0b01, 1, 1, 190, 90
    inputs, upto, phases, _ = assembled(P, mask, rd, n, ticks)
    di, du = dev(inputs, upto)
    dr = {p: dev(r) for p, r in phases.items()}
    cls = Cohorts(game, P, d, rd, mask, n, sparse=sparse)
    for t in range(ticks):
        if t in RESTARTS:
            cls.restart(RESTARTS[t])
        cls.tick(t, ALL, inputs, upto, phases[phase_of(t)])
    ends = {}
    for chunk in (1, 7, 50):  # kOne, kQ, LdsC|Async
        sess = start(game, P, mask, d, rd, sparse, n)
        for t in range(t_split):
            if t in RESTARTS:
                sess.restart_sessions(cohort_mask(n, RESTARTS[t]))
            sess.run_ticks(di[t:t + 1], du[t:t + 1], dr[phase_of(t)])
        sess.restart_sessions(cohort_mask(n, RESTARTS[t_split]))
        for t0 in range(t_split, ticks, chunk):
            t1 = min(ticks, t0 + chunk)
            sess.run_ticks(di[t0:t1], du[t0:t1], dr[t_split])
        compare_all(sess, cls, f"{case}, launches of {chunk}")
        ends[chunk] = everything(sess, False)
        sess.close()
    for chunk in (7, 50):
        for k in ends[1]:
            if k not in ("lf", "na", "ns"):  # the last tick's own requests are compared with the oracle above
                np.testing.assert_array_equal(ends[chunk][k], ends[1][k], err_msg=f"{k}, launches of {chunk} against 1")
    cur = ends[1]["cur"]
    assert cur[0::3].min() - cur[2::3].max() > 60
    cls.close()


# ---------------------------------------------------------------------------
# GPU 5: the escape rows
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_restart_clears_the_escape_rows(gpu_available):
    """Player 1 is disconnected at tick 30; past frame 32,800 its frozen frames sit behind the escape
    bit in the absolute rows.  Odd sessions are restarted and play a second match; the even ones go
    on.  The restarted sessions equal a fresh batch's, the others an unrestarted twin's."""
    P, mask, d, rd, n, t_long, more = 2, 0b01, 1, 1, 12, 32800, 40
    inputs, upto, rin = synth_network(n, P, t_long + more, mask, rd, 1, 5)
    upto[30:, 1] = upto[29, 1]
    second = synth_network(n, P, more, mask, rd, 1, 4, seed=SEED ^ 0xE5C)
    odd = np.arange(n) % 2 == 1
    a, twin, fresh = (make_session(G.Game.EX_GAME, P, mask, d, rd, sessions=n, time_sync=False) for _ in range(3))
    di, du, dr = dev(inputs, upto, rin)
    for t0 in [0, 30] + list(range(50, t_long, 50)):
        t1 = 30 if t0 == 0 else min(t_long, 50 if t0 == 30 else t0 + 50)
        for b in (a, twin):
            if t0 == 30:
                b.disconnect_player(1)
            b.run_ticks(di[t0:t1], du[t0:t1], dr)
    assert (a.frames()[0] - a.read_queues()[:, 1, 0] > 32767).all(), "every session's player 1 escaped"
    a.restart_sessions(odd)
    # the restarted batch's tensors: the odd columns play the second match from its tick 0
    mi = inputs[t_long:t_long + more].copy()
    mu = upto[t_long:t_long + more].copy()
    mr = rin.copy()
    mi[:, :, odd], mu[:, :, odd] = second[0][:, :, odd], second[1][:, :, odd]
    mr[:more + rd][:, :, odd] = second[2][:, :, odd]
    ai, au, ar = dev(mi, mu, mr)
    fi, fu, fr = dev(*second)
    for t in range(more):
        a.run_ticks(ai[t:t + 1], au[t:t + 1], ar)
        twin.run_ticks(di[t_long + t:t_long + t + 1], du[t_long + t:t_long + t + 1], dr)
        fresh.run_ticks(fi[t:t + 1], fu[t:t + 1], fr)
        got, old, new = (everything(b, False) for b in (a, twin, fresh))
        for k in got:
            if k in ("totals", "counters"):
                continue
            ax = 1 if k in ("tags", "imgs", "cs") else 0
            np.testing.assert_array_equal(np.compress(odd, got[k], ax), np.compress(odd, new[k], ax), err_msg=f"{k}, restarted, tick {t}")
            np.testing.assert_array_equal(np.compress(~odd, got[k], ax), np.compress(~odd, old[k], ax), err_msg=f"{k}, kept, tick {t}")
    q = a.read_queues()
    assert (q[odd, 1, 7] == 0).all() and (q[~odd, 1, 7] == 1).all() and (a.frames()[0][odd] > 20).all()
    assert a.counters()[2] == 0
    for b in (a, twin, fresh):
        b.close()


# ---------------------------------------------------------------------------
# GPU 6: a panicked slot runs again
# ---------------------------------------------------------------------------
def compare_rows(sess, orc, last, rows, what):
    """compare_all against a plain oracle of the same width (`last`: its advance()), on the sessions
    `rows` only."""
    st, lf, na, ns = sess.status()
    ost, olf, ona, ons = last
    for x, y, name in ((st, ost, "status"), (lf, olf, "load frame"), (na, ona, "advances"), (ns, ons, "saves")):
        np.testing.assert_array_equal(x[rows], y[rows], err_msg=f"{name}, {what}")
    tags, imgs, cs = sess.read_cells()
    otags, oimgs, ocs = orc.read_cells()
    np.testing.assert_array_equal(tags[:, rows], otags[:, rows], err_msg=f"cell frames, {what}")
    valid = (otags >= 0) & rows[None, :]
    np.testing.assert_array_equal(imgs[valid], oimgs[valid], err_msg=f"cell images, {what}")
    np.testing.assert_array_equal(cs[valid], ocs[valid], err_msg=f"cell checksums, {what}")
    np.testing.assert_array_equal(sess.read_live()[rows], orc.read_live()[0][rows], err_msg=f"live, {what}")
    for x, y in zip(sess.frames(), orc.frames()):
        np.testing.assert_array_equal(x[rows], y[rows], err_msg=f"frames, {what}")
    dq, oq = sess.read_queues(), orc.queues()
    dq[:, :, 1] = np.where(dq[:, :, 0] < 0, oq[:, :, 1], dq[:, :, 1])
    np.testing.assert_array_equal(dq[rows], oq[rows], err_msg=f"queues, {what}")


@pytest.mark.gpu
def test_gpu_a_panicked_session_runs_again_after_its_restart(gpu_available):
    """test_p2p_pacing.py's overflow: the sessions s % 4 == 3 are parked for 135 ticks while a frame
    is delivered every tick, and panic inside a parked poll (input_queue.rs:181)."""
    P, mask, d, rd, ticks, more = 2, 0b01, 0, 0, 150, 40
    inputs, _, rin = synth_network(S, P, ticks + more, mask, rd, 1, 1)
    upto = np.full((ticks + more, P, S), -1, np.int32)
    upto[:, 1, :] = np.arange(ticks + more)[:, None] - 1
    victims = np.arange(S) % 4 == 3
    masks = np.ones((ticks, S), np.uint8)
    masks[10:145, victims] = 0
    second = synth_network(S, P, more, mask, rd, 1, 4, seed=SEED ^ 0x9A1C)
    sess = make_session(G.Game.EX_GAME, P, mask, d, rd, time_sync=False)
    di, du, dr, dm = dev(inputs, upto, rin, masks)
    sess.run_ticks(di[:ticks], du[:ticks], dr, run_mask=dm)
    st = sess.status()[0]
    assert (st[victims] == L.RB_PANIC).all() and (st[~victims] == 0).all()
    counters = sess.counters()
    assert counters[2] == victims.sum()
    frozen = snapshot(sess)
    sess.restart_sessions(victims)
    assert sess.counters() == counters, "the panic count is the batch's, since create"
    assert (sess.status()[0] == 0).all() and (sess.parked_ticks()[victims] == 0).all()
    assert (sess.parked_ticks()[~victims] == 0).all()
    for x, y in zip(frozen, snapshot(sess)):
        ax = 1 if x.ndim > 1 and x.shape[0] == W else 0
        np.testing.assert_array_equal(np.compress(~victims, x, ax), np.compress(~victims, y, ax))
    mi, mu, mr = inputs[ticks:].copy(), upto[ticks:].copy(), rin.copy()
    mi[:, :, victims], mu[:, :, victims] = second[0][:, :, victims], second[1][:, :, victims]
    mr[:more + rd][:, :, victims] = second[2][:, :, victims]
    ai, au, ar = dev(mi, mu, mr)
    orc = O.OracleP2P(O.EX_GAME, P, W, d, mask, S, remote_delay=rd)
    for t in range(more):
        sess.run_ticks(ai[t:t + 1], au[t:t + 1], ar)
        assert orc.deliver(1, np.ascontiguousarray(second[1][t, 1]), np.ascontiguousarray(second[2][:, 1])) == 0
        orc.add_local_input(0, np.ascontiguousarray(second[0][t, 0]))
        last = orc.advance()
        compare_rows(sess, orc, last, victims, f"tick {t} after the restart")
    assert (sess.status()[0] != L.RB_PANIC).all() and sess.counters()[2] == counters[2]
    assert (sess.frames()[0][victims] > 20).all() and (sess.frames()[0][~victims] == ticks + more).all()
    orc.close()
    sess.close()


# ---------------------------------------------------------------------------
# GPU 7: packet-fed ticks
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_packet_fed_ticks_with_cohort_restarts_equal_direct_delivery(gpu_available):
    """The packets of a restarted session start again at frame 0: its sender knows nothing acked."""
    import torch
    lib = L.load()
    P, mask, d, rd, stride = 2, 0b01, 1, 2, 32
    inputs, upto, phases, _ = assembled(P, mask, rd)
    di, du = dev(inputs, upto)
    dr = {p: dev(r) for p, r in phases.items()}
    rng = np.random.default_rng(7)
    pk = torch.zeros((T, P, S, stride), dtype=torch.uint8, device="cuda")
    ln = torch.zeros((T, P, S), dtype=torch.int32, device="cuda")
    sf = torch.zeros((T, P, S), dtype=torch.int32, device="cuda")
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    for t in range(T):  # tests/test_wire.py _encode_schedule, with the acked frame of a new match NULL
        prev = upto[t - 1, 1].copy() if t > 0 else np.full(S, -1, np.int32)
        if t in RESTARTS:
            prev[cohort_mask(S, RESTARTS[t]) != 0] = -1
        acked = np.where(prev < 0, prev, np.maximum(prev - rng.integers(0, 3, S), rd - 1))
        acked = dev(np.where(acked < rd, -1, acked).astype(np.int32))
        rin = dr[phase_of(t)]
        assert lib.rb_encode_input_packets(0, None, 1, P, S, 1, p(rin), int(rin.shape[0]), rd, p(acked), p(du[t, 1].contiguous()),
                                           p(pk[t, 1]), stride, p(ln[t, 1]), p(sf[t, 1])) == 0
    torch.cuda.synchronize()
    assert int((ln < 0).sum()) == 0
    wired, direct = (make_session(G.Game.EX_GAME, P, mask, d, rd, time_sync=False) for _ in range(2))
    for t in range(T):
        if t in RESTARTS:
            for b in (wired, direct):
                b.restart_sessions(cohort_mask(S, RESTARTS[t]))
        wired.run_ticks_packets(di[t:t + 1], pk[t:t + 1], ln[t:t + 1], sf[t:t + 1])
        direct.run_ticks(di[t:t + 1], du[t:t + 1], dr[phase_of(t)])
        want, got = everything(direct, False), everything(wired, False)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k}, tick {t}")
    assert wired.counters()[2] == 0
    cur = wired.frames()[0]
    assert cur[0::3].min() > cur[1::3].max() > cur[2::3].max()
    wired.close()
    direct.close()


# ---------------------------------------------------------------------------
# GPU 8: spectators
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_spectators_restart_with_their_hosts(gpu_available):
    """DESIGN.md section 11's identity for every match of every cohort: the spectator's state after
    frame c is the host's cell of frame c + 1."""
    from test_spectator import DELAY, REMOTE_DELAY, W_, Feed, start_host, start_spectators
    game, P, mask = G.Game.EX_GAME, 2, 0b01
    inputs, upto, phases, _ = assembled(P, mask, REMOTE_DELAY)
    di, du = dev(inputs, upto)
    dr = {p: dev(r) for p, r in phases.items()}
    host, spec = start_host(game, P, mask, S), start_spectators(game, P, S)
    feed = Feed(host, T + DELAY + 4)
    co = cohort_of(S)
    compared = {}
    spec_totals = None
    for t in range(T):
        if t in RESTARTS:
            sel = cohort_mask(S, RESTARTS[t])
            spec_totals = spec.totals()
            host.restart_sessions(sel)
            spec.restart_sessions(sel)
            assert spec.totals() == spec_totals
            cur, recv = spec.frames()
            assert (cur[sel != 0] == -1).all() and (recv[sel != 0] == -1).all() and (cur[sel == 0] > 10).all()
            assert (host.export_status()[1][sel != 0] == 0).all() and (host.export_status()[1][sel == 0] > 10).all()
        host.run_ticks(di[t:t + 1], du[t:t + 1], dr[phase_of(t)])
        host.export_confirmed_inputs(feed.inputs, feed.upto, feed.last, feed.disc)
        spec.receive_host_status(feed.last.clone(), feed.disc.clone())
        spec.run_ticks(feed.upto.clone()[None], feed.inputs)
        if t % 6 == 5 or t + 1 in RESTARTS or t == T - 1:
            cur, _ = spec.frames()
            img, cs = spec.read_live()
            tags, himg, hcs = host.read_cells()
            conf = host.frames()[1]
            for s in range(S):
                f = int(cur[s]) + 1
                if tags[f % W_, s] == f and f <= conf[s]:
                    assert np.array_equal(img[s], himg[f % W_, s]) and np.array_equal(cs[s], hcs[f % W_, s]), f"tick {t} session {s}"
                    key = (int(co[s]), match_start(int(co[s]), t))
                    compared[key] = compared.get(key, 0) + 1
    assert set(compared) == {(0, 0), (1, 0), (1, 37), (2, 0), (2, 37), (2, 90)}, compared
    assert (host.export_status()[0] == L.RB_P2P_EXPORT_OK).all() and host.counters()[2] == 0
    cur = spec.frames()[0]
    assert cur[0::3].min() > cur[1::3].max() and cur[1::3].min() > cur[2::3].max() and cur.min() > 20
    host.close()
    spec.close()


@pytest.mark.gpu
def test_gpu_an_overrun_export_starts_again_after_the_restart(gpu_available):
    from test_spectator import Feed, expected_by_frame, host_network, start_host
    game, P, mask, more = G.Game.EX_GAME, 2, 0b01, 20
    inputs, upto, rin = host_network(game, P, mask, S, 140)
    host = start_host(game, P, mask, S)
    host.run_ticks(*dev(inputs, upto, rin))
    Feed(host, 160).export()
    assert (host.export_status()[0] == L.RB_P2P_EXPORT_OVERRUN).all()
    sel = np.arange(S) % 2 == 0
    host.restart_sessions(sel)
    est, nxt = host.export_status()
    np.testing.assert_array_equal(est, np.where(sel, L.RB_P2P_EXPORT_OK, L.RB_P2P_EXPORT_OVERRUN))
    assert (nxt == 0).all()
    second = synth_network(S, P, more, mask, 1, 1, 3, seed=SEED ^ 0x0E)
    host.run_ticks(*dev(*second))  # (the sessions not restarted are fed frames they long hold: ignored)
    feed = Feed(host, more + 8)
    got, gup, _, _ = feed.export()
    want, known = expected_by_frame(P, mask, second[0], second[2], more + 8)
    est, nxt = host.export_status()
    np.testing.assert_array_equal(est, np.where(sel, L.RB_P2P_EXPORT_OK, L.RB_P2P_EXPORT_OVERRUN))
    assert (gup[sel] > 8).all() and (nxt[sel] == gup[sel] + 1).all() and (gup[~sel] == -1).all()
    for s in np.nonzero(sel)[0]:
        u = int(gup[s])
        for h in range(P):
            k = known[:u + 1, h]
            assert np.array_equal(got[:u + 1, h, s][k], want[:u + 1, h, s][k]), f"session {s} handle {h}"
        assert (got[u + 1:, :, s] == feed.sentinel).all()
    assert (got[:, :, ~sel] == feed.sentinel).all()
    host.close()


# ---------------------------------------------------------------------------
# GPU 9: validation and no-ops
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_empty_selections_early_restarts_and_user_streams(gpu_available):
    import torch
    P, mask, d, rd = 2, 0b01, 1, 1
    inputs, upto, rin = synth_network(S, P, 40, mask, rd, 1, 4)
    di, du, dr = dev(inputs, upto, rin)
    sess, twin = (make_session(G.Game.EX_GAME, P, mask, d, rd) for _ in range(2))

    def same(what):
        want, got = everything(twin, True), everything(sess, True)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k}, {what}")

    sess.restart_sessions(None)  # before the first tick: a no-op by content
    sess.restart_sessions(np.arange(S) % 2 == 0)
    same("restarts before the first tick")
    for b in (sess, twin):
        b.run_ticks(di[:20], du[:20], dr)
    sess.profile_enable(True)
    sess.restart_sessions(np.zeros(S, np.uint8))  # an empty selection: nothing changes, nothing is launched
    sess.restart_sessions(False)
    assert sess.profile_take()[1] == 0
    sess.profile_enable(False)
    same("an all-zero mask")
    with pytest.raises(ValueError):
        sess.restart_sessions(np.zeros(S + 1, np.uint8))
    with pytest.raises(G.InvalidRequest):  # the batch still validates like before: time sync stays closed
        sess.enable_time_sync(60)
    same("refused calls")
    # on a user stream: the restart is ordered between the ticks around it
    stream = torch.cuda.Stream()
    sess.set_stream(stream)
    sel = np.arange(S) % 3 == 1
    with torch.cuda.stream(stream):
        sess.run_ticks(di[20:30], du[20:30], dr)
        sess.restart_sessions(sel)
        sess.run_ticks(di[:10], du[:10], dr)
    fresh = make_session(G.Game.EX_GAME, P, mask, d, rd)
    fresh.run_ticks(di[:10], du[:10], dr)
    want, got = everything(fresh, True), everything(sess, True)
    for k in want:
        if k not in ("totals", "counters"):
            ax = 1 if k in ("tags", "imgs", "cs") else (want[k].ndim - 1 if k in ("local_adv", "remote_adv", "rtt", "windows") else 0)
            np.testing.assert_array_equal(np.compress(sel, got[k], ax), np.compress(sel, want[k], ax), err_msg=f"{k}, user stream")
    assert (sess.frames()[0][sel] <= 10).all() and (sess.frames()[0][~sel] >= 28).all()
    from test_spectator import start_spectators
    spec = start_spectators(G.Game.EX_GAME, P, S)
    before = spec.frames() + spec.status() + spec.read_live()
    spec.restart_sessions(np.zeros(S, bool))
    spec.restart_sessions(None)
    for x, y in zip(before, spec.frames() + spec.status() + spec.read_live()):
        np.testing.assert_array_equal(x, y)
    for b in (sess, twin, fresh, spec):
        b.close()
