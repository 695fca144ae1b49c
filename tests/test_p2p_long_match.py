"""P2P paths against the oracle past the input ring's wrap.

InputQueue is a 128-entry ring (input_queue.rs:6); on the device every input
read and write goes through ``f & 127`` (p2p.hpp RingIO, LdsRing, the LDS
copy-in and write-back at launch edges, rb_p2p_export_confirmed_inputs), and
q_discard's three tail branches only separate once a queue has seen 126, 127
or more frames.  Every test here runs 300 ticks, so frames 128 and 256 are
crossed (the ring wrapped once and twice), with launch edges on both sides of
a multiple of 128:

  live   300 one-tick calls (kOne; Wire|One when packet-fed)
  q      calls of 7 ticks: [119,126) and [126,133) straddle 127/128, [252,259) 256
  cells  calls of 29 ticks: [116,145) and [232,261) straddle the wraps

After every call the last tick's status, LoadGameState frame, AdvanceFrame and
SaveGameState counts equal the oracle's; cells, live state, frames and every
InputQueue's bookkeeping (compare_state) after every fused call, and in the
live plan at every tick of [120, 136] and [250, 262], every 25 ticks elsewhere
and at the last tick.  Every comparison is bit-exact equality.

The disconnect and peer-report schedules sit on the ring's edges (a player
leaving with 126, 127 or more frames in its queue); CPU witnesses drive the
oracle alone through them and assert that the edges are really reached.
"""
import functools

import numpy as np
import pytest

import ggrs_amd as G
from ggrs_amd._lib import RB_P2P_EVENTS_KEPT, RB_PANIC
from ggrs_amd.p2p import PlayerType, synth_network
from oracle import oracle as O
from test_p2p import ORC_GAME, compare_queues, compare_state, drive_oracle, gpu_pair
from test_p2p_desync import (MASK_A, MASK_B, dev_reports_as_oracle, exchange_oracle, gpu_peer, networks, oracle_peer,
                             oracle_tick)
from test_p2p_peer_status import drive as peer_drive
from test_wire import _encode_schedule, _oracle_packet_deliveries

T, S, S_BRAWLER, W = 300, 70, 48, 8
WRAP = 128  # kQueueLen
LIVE_WINDOWS = set(range(120, 137)) | set(range(250, 263))
PLAN_TICKS = {"live": 1, "q": 7, "cells": 29, "cells-lockstep": 29}


def plan_calls(plan, upto=T, t0=0):
    n = PLAN_TICKS[plan]
    return [(a, min(a + n, upto)) for a in range(t0, upto, n)]


def wants_state(t0, t1):
    """compare_state after this call?  Every fused call; one-tick calls inside the windows
    around the wraps, every 25 ticks elsewhere and at the last tick."""
    t = t1 - 1
    return t1 - t0 > 1 or t in LIVE_WINDOWS or t % 25 == 24 or t == T - 1


def net_for(game, S_, P, mask, rd, lag, imask=None):
    dt = np.uint32 if game == G.Game.STUB else np.uint8
    if imask is None:
        imask = {G.Game.STUB: 0x3, G.Game.STUB_ENUM: 0x1}.get(game, 0x0F)
    return synth_network(S_, P, T, mask, rd, lag[0], lag[1], dtype=dt, mask=imask)


def run_against_oracle(sess, orc, mask, net, calls, disc=None, state=wants_state):
    """The calls [(t0, t1)] on the device and the same ticks on the oracle; after every call the
    last tick's status, rollback frame and request counts, and the state where `state` asks.
    disc: {tick: [(handle, session mask)]} disconnect_player calls before that tick (a call must
    start there).  A session the oracle panics is dead from then on (test_p2p.py's `alive`).
    Returns (alive, rolled back at a call's last tick >= 128)."""
    import torch
    inputs, upto, rin = net
    di, du, dr = (torch.from_numpy(a).cuda() for a in net)
    disc = disc or {}
    assert set(disc) <= {c[0] for c in calls}, "a disconnect must sit between two calls"
    alive = np.ones(inputs.shape[2], bool)
    rolled_after_wrap = False
    for t0, t1 in calls:
        for h, m in disc.get(t0, []):
            sess.disconnect_player(h, m)
        sess.run_ticks(di[t0:t1], du[t0:t1], dr)
        ost, olf, ona, ons = drive_oracle(orc, mask, inputs, upto, rin, t1, t0=t0, disc=disc)[-1]
        st, lf, na, ns = sess.status()
        st = np.where(st == RB_PANIC, O.KIND_PANIC, st)
        np.testing.assert_array_equal(st[alive], ost[alive], err_msg=f"status, tick {t1 - 1}")
        alive &= ost != O.KIND_PANIC
        np.testing.assert_array_equal(lf[alive], olf[alive], err_msg=f"LoadGameState frame, tick {t1 - 1}")
        np.testing.assert_array_equal(na[alive], ona[alive], err_msg=f"AdvanceFrame count, tick {t1 - 1}")
        np.testing.assert_array_equal(ns[alive], ons[alive], err_msg=f"SaveGameState count, tick {t1 - 1}")
        if t1 - 1 >= WRAP:
            rolled_after_wrap |= bool((lf[alive] != G.NULL_FRAME).any())
        if state(t0, t1):
            compare_state(sess, orc, t1 - 1, alive)
    assert calls[-1][1] == T
    return alive, rolled_after_wrap


# ---------------------------------------------------------------------------- 1. the long-match matrix
def _rows():
    E, ST, SE, B = G.Game.EX_GAME, G.Game.STUB, G.Game.STUB_ENUM, G.Game.BRAWLER
    both = ("cells", "cells-lockstep")
    rows = [  # game, P, mask, W, sparse, d, rd, lag, fan-out (None / "one" / "per-player"), plans
        (E, 2, 0b01, 8, False, 2, 2, (0, 6), None, ("q",)),
        (E, 3, 0b010, 7, True, 0, 2, (0, 4), None, ("live", "q") + both),
        (E, 4, 0b0001, 8, False, 1, 1, (1, 5), None, both),
        (E, 2, 0b01, 12, False, 1, 1, (1, 9), None, ("cells",)),  # W > 8: HBM cells
        (E, 4, 0b0001, 8, False, 1, 1, (1, 5), "per-player", ("live", "cells")),
        (E, 4, 0b0001, 8, False, 1, 1, (1, 5), "one", ("live", "cells")),
        (ST, 2, 0b01, 8, False, 1, 0, (1, 5), None, ("live", "cells")),  # u32 inputs, HBM ring
        (ST, 2, 0b01, 8, True, 1, 0, (1, 5), None, ("live", "cells")),
        (SE, 2, 0b10, 6, True, 0, 2, (0, 5), None, ("live",)),
        (B, 2, 0b01, 8, False, 1, 1, (1, 4), None, ("live", "q")),
        (B, 2, 0b10, 6, True, 0, 2, (0, 5), None, ("q",)),
    ]
    return [r[:9] + (plan,) for r in rows for plan in r[9]]


MATRIX = _rows()


def _matrix_id(c):
    game, P, mask, W_, sparse, d, rd, lag, fan, plan = c
    return f"{game.name}-P{P}-m{mask}-W{W_}-sp{int(sparse)}-d{d}-rd{rd}-{'fo-' + fan + '-' if fan else ''}{plan}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", MATRIX, ids=[_matrix_id(c) for c in MATRIX])
def test_gpu_long_match_matches_oracle(gpu_available, monkeypatch, case):
    game, P, mask, W_, sparse, d, rd, lag, fan, plan = case
    if plan.startswith("cells"):  # lane-asynchronous ticks unless lock-step (test_gpu_p2p_fused_launches_match_oracle)
        monkeypatch.setenv("RB_P2P_SYNC_TICKS", "1" if plan == "cells-lockstep" else "0")
    S_ = S_BRAWLER if game == G.Game.BRAWLER else S
    net = net_for(game, S_, P, mask, rd, lag)
    sess, orc = gpu_pair(game, S_, P, W_, d, rd, mask, sparse, fanout=fan is not None, per_player=fan == "per-player")
    alive, rolled = run_against_oracle(sess, orc, mask, net, plan_calls(plan))
    assert alive.all() and sess.counters()[2] == 0
    assert rolled, "no rollback after the ring wrapped"
    assert (sess.frames()[0] > 2 * WRAP).all()
    if fan:  # the oracle knows no fan-out: a select must be observably the reference's rollback
        adv, saves, loads, selects, branch_frames = sess.totals()
        assert selects > 0 and branch_frames > 0 and sess.counters()[1] == 0
    sess.close()


@pytest.mark.gpu
def test_gpu_long_match_plugin_game_matches_oracle(gpu_available):
    # the orbit game of test_gpu_plugin_p2p_matches_oracle_every_tick (it folds InputStatus into its state)
    from ggrs_amd.plugin import register_game_plugin
    from test_plugin_game import ORC, PLUGIN
    P, mask, d, rd, lag = 3, 0b001, 1, 2, (1, 4)
    gid = register_game_plugin(PLUGIN)
    net = synth_network(S, P, T, mask, rd, lag[0], lag[1], mask=0x1F)
    b = (G.SessionBuilder(gid, num_sessions=S).with_num_players(P).with_max_prediction_window(W)
         .with_input_delay(d).with_remote_input_delay(rd))
    for h in range(P):
        b.add_player(PlayerType.Local if (mask >> h) & 1 else PlayerType.Remote, h)
    sess = b.start_p2p_session()
    orc = O.OracleP2P(O.PLUGIN, P, W, d, mask, S, remote_delay=rd, lib_path=ORC)
    alive, rolled = run_against_oracle(sess, orc, mask, net, plan_calls("live"))
    assert alive.all() and sess.counters()[2] == 0 and rolled
    sess.close()


# ---------------------------------------------------------------------------- 2. disconnects at the ring's edges
def edge_disconnects(S_, first, second):
    """{tick: [(handle, session mask)]}: `first` leaves sessions s % 20 == k before tick 118 + k,
    `second` leaves sessions s % 12 == k before tick 250 + k."""
    s = np.arange(S_)
    disc = {}
    for k in range(20):
        disc.setdefault(118 + k, []).append((first, s % 20 == k))
    for k in range(12 if second is not None else 0):
        disc.setdefault(250 + k, []).append((second, s % 12 == k))
    return disc


def edge_calls(fused):
    """One-tick calls through [110, 140] and [245, 265] (the disconnects sit between calls),
    calls of `fused` ticks elsewhere."""
    calls = []
    for a, b, n in ((0, 110, fused), (110, 141, 1), (141, 245, fused), (245, 266, 1), (266, T, fused)):
        calls += [(t, min(t + n, b)) for t in range(a, b, n)]
    return calls


EDGE_WINDOWS = set(range(110, 141)) | set(range(245, 266))
EDGE_CASES = [  # game, P, mask, sparse, fan-out, lag, sessions, ticks per fused call
    (G.Game.EX_GAME, 3, 0b001, False, False, (1, 5), S, 29),
    (G.Game.EX_GAME, 3, 0b001, True, False, (1, 5), S, 29),
    # the stub games have two players (tests/stubs.rs: p0_inputs + p1_inputs; the batch refuses any other
    # count): the only remote player leaves by the first rule, nobody is left for the second
    (G.Game.STUB, 2, 0b01, False, False, (1, 5), S, 29),
    (G.Game.BRAWLER, 3, 0b001, False, False, (1, 4), S_BRAWLER, 29),
    (G.Game.EX_GAME, 4, 0b0001, False, True, (1, 5), S, 29),
    (G.Game.EX_GAME, 3, 0b001, False, False, (1, 5), S, 7),
]
EDGE_IDS = [f"{c[0].name}-P{c[1]}-sp{int(c[3])}-fo{int(c[4])}-tpl{c[7]}" for c in EDGE_CASES]
EDGE_D = EDGE_RD = 1


def edge_handles(P):
    return P - 1, (P - 2 if P > 2 else None)  # the first and the second player to leave


def test_edge_disconnect_schedule_reaches_the_ring_edges_on_the_oracle():
    """The witness of test_gpu_disconnects_at_the_ring_edges_match_oracle: the oracle alone through
    each schedule.  The first player to leave must do so with 126, with 127, with fewer and with
    more frames in its queue, with NULL and with real tails (q_discard's delete-all branch on both
    sides of a full ring); the second leaves after the wrap with a positive tail."""
    seen = set()
    for game, P, mask, sparse, _, lag, S_, _ in EDGE_CASES:
        if (game, P, sparse) in seen:  # (the 7-tick launch plan shares its schedule)
            continue
        seen.add((game, P, sparse))
        first, second = edge_handles(P)
        inputs, upto, rin = net_for(game, S_, P, mask, EDGE_RD, lag)
        orc = O.OracleP2P(ORC_GAME[game], P, W, EDGE_D, mask, S_, sparse_saving=sparse, remote_delay=EDGE_RD)
        res = drive_oracle(orc, mask, inputs, upto, rin, T, disc=edge_disconnects(S_, first, second))
        what = f"{game.name} P{P} sparse {sparse}"
        assert all((r[0] != O.KIND_PANIC).all() for r in res), what
        q = orc.queues()
        last_added, tail = q[:, first, 0], q[:, first, 1]
        assert (last_added == WRAP - 2).any() and (last_added == WRAP - 1).any(), (what, sorted(set(last_added)))
        assert (last_added < WRAP - 2).any() and (last_added > WRAP - 1).any(), (what, sorted(set(last_added)))
        assert (tail == G.NULL_FRAME).any() and (tail >= 0).any(), (what, sorted(set(tail)))
        assert (q[:, first, 7] != 0).all()  # disconnected everywhere
        if second is not None:
            assert (q[:, second, 1] >= 100).all(), (what, sorted(set(q[:, second, 1])))
            assert (q[:, second, 7] != 0).all()
        orc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", EDGE_CASES, ids=EDGE_IDS)
def test_gpu_disconnects_at_the_ring_edges_match_oracle(gpu_available, case):
    game, P, mask, sparse, fanout, lag, S_, fused = case
    first, second = edge_handles(P)
    net = net_for(game, S_, P, mask, EDGE_RD, lag)
    sess, orc = gpu_pair(game, S_, P, W, EDGE_D, EDGE_RD, mask, sparse, fanout=fanout)
    alive, rolled = run_against_oracle(sess, orc, mask, net, edge_calls(fused), disc=edge_disconnects(S_, first, second),
                                       state=lambda t0, t1: t1 - t0 > 1 or t1 - 1 in EDGE_WINDOWS or t1 == T)
    assert alive.all() and sess.counters()[2] == 0  # (the witness: the oracle panics nowhere)
    assert rolled
    q = sess.read_queues()
    assert (q[:, first, 0] == WRAP - 2).any() and (q[:, first, 0] == WRAP - 1).any()
    sess.close()


# ---------------------------------------------------------------------------- 3. peer-reported disconnects at the edge
PEER_P, PEER_MASK, PEER_D, PEER_RD, PEER_LAG = 3, 0b001, 1, 2, (1, 3)  # test_p2p_peer_status.py
PEER_TICKS = range(124, 132)


def edge_reports(S_, upto, t):
    """The connect-status reports given before tick t (test_p2p_peer_status.reports' shape):
    endpoint 2 reports player 1 disconnected at the frame we hold in the group of 8 sessions whose
    tick t is (group g before tick 124 + g); everything else is a plain connected report."""
    held = upto[t]
    out = []
    for e in (1, 2):
        last = np.full((PEER_P, S_), -1, np.int32)
        disc = np.zeros((PEER_P, S_), np.uint8)
        for i in range(PEER_P):
            last[i] = np.maximum(held[i] if i != 0 else t - 1 + PEER_D, -1)
        if e == 2 and t in PEER_TICKS:
            g = t - PEER_TICKS[0]
            disc[1, 8 * g:8 * g + 8] = 1
        out.append((e, last, disc))
    return out


def reported_frames(S_, upto):
    """The frame each session's report names for player 1 (NULL_FRAME: never reported)."""
    f = np.full(S_, G.NULL_FRAME, np.int32)
    for t in PEER_TICKS:
        g = t - PEER_TICKS[0]
        f[8 * g:8 * g + 8] = upto[t, 1, 8 * g:8 * g + 8]
    return f


@pytest.mark.parametrize("sparse", [False, True])
def test_edge_peer_reports_name_frames_126_and_127_on_the_oracle(sparse):
    """The witness of test_gpu_peer_reported_disconnects_at_the_ring_edge_match_oracle.  A report
    naming frame F = current_frame - 1 sets disconnect_frame to the current frame, which the
    reference's load_frame refuses (sync_layer.rs:141-145; test_p2p_peer_status.py): those sessions
    panic in the reference too, at the report's tick, and no session panics for another reason or
    at another tick.  Frames 126 and 127 must both be reported in sessions that live on."""
    inputs, upto, rin = synth_network(S, PEER_P, T, PEER_MASK, PEER_RD, *PEER_LAG)
    orc = O.OracleP2P(O.EX_GAME, PEER_P, W, PEER_D, PEER_MASK, S, sparse_saving=sparse, remote_delay=PEER_RD)
    frames = reported_frames(S, upto)
    group = lambda t: slice(8 * (t - PEER_TICKS[0]), 8 * (t - PEER_TICKS[0]) + 8)
    panicked = np.zeros(S, bool)
    for t in range(T):
        if t in PEER_TICKS:
            for e, last, disc in edge_reports(S, upto, t):
                orc.receive_peer_connect_status(e, last, disc)
            cur = orc.frames()[0].copy()
        pan = peer_drive(orc, inputs, upto, rin, t)[0] == O.KIND_PANIC
        new = pan & ~panicked
        if new.any():
            assert t in PEER_TICKS and not np.delete(new, np.r_[group(t)]).any(), f"a panic outside tick {t}'s group"
            assert (frames[new] == cur[new] - 1).all(), (t, frames[new], cur[new])
        panicked |= pan
    for f in (WRAP - 2, WRAP - 1):
        assert (frames == f).any(), sorted(set(frames))
        assert (~panicked[frames == f]).any(), (f, np.nonzero(panicked)[0])
    q = orc.queues()
    live = ~panicked
    assert (q[:64, 1, 7][live[:64]] != 0).all() and (q[64:, 1, 7] == 0).all()  # the reports took effect, and only there
    assert live[64:].all() and live[:64].sum() >= 16


@pytest.mark.gpu
@pytest.mark.parametrize("sparse", [False, True])
def test_gpu_peer_reported_disconnects_at_the_ring_edge_match_oracle(gpu_available, sparse):
    # the kNet kernels; compared as test_gpu_peer_reported_disconnects_match_oracle_every_tick does
    import torch
    inputs, upto, rin = synth_network(S, PEER_P, T, PEER_MASK, PEER_RD, *PEER_LAG)
    b = (G.SessionBuilder(G.Game.EX_GAME, num_sessions=S).with_num_players(PEER_P).with_max_prediction_window(W)
         .with_input_delay(PEER_D).with_remote_input_delay(PEER_RD).with_sparse_saving_mode(sparse)
         .with_peer_connect_status(True))
    for h in range(PEER_P):
        b.add_player(PlayerType.Local if (PEER_MASK >> h) & 1 else PlayerType.Remote, h)
    sess = b.start_p2p_session()
    orc = O.OracleP2P(O.EX_GAME, PEER_P, W, PEER_D, PEER_MASK, S, sparse_saving=sparse, remote_delay=PEER_RD)
    di, du, dr = (torch.from_numpy(a).cuda() for a in (inputs, upto, rin))
    alive = np.ones(S, bool)
    rolled = False
    for t in range(T):
        if t in PEER_TICKS:
            for e, last, disc in edge_reports(S, upto, t):
                orc.receive_peer_connect_status(e, last, disc)
                sess.receive_peer_connect_status(e, torch.from_numpy(last).cuda(), torch.from_numpy(disc).cuda())
        sess.run_ticks(di[t:t + 1], du[t:t + 1], dr)
        ost, olf, ona, ons = peer_drive(orc, inputs, upto, rin, t)
        st, lf, na, ns = sess.status()
        np.testing.assert_array_equal(st, np.where(ost == O.KIND_PANIC, RB_PANIC, ost), err_msg=f"status, tick {t}")
        alive &= ost != O.KIND_PANIC
        np.testing.assert_array_equal(lf[alive], olf[alive], err_msg=f"load frame, tick {t}")
        np.testing.assert_array_equal(na[alive], ona[alive], err_msg=f"AdvanceFrames, tick {t}")
        np.testing.assert_array_equal(ns[alive], ons[alive], err_msg=f"SaveGameStates, tick {t}")
        compare_queues(sess, orc, t, alive)
        rolled |= t >= WRAP and bool((lf[alive] != G.NULL_FRAME).any())
        if t % 5 == 4:
            np.testing.assert_array_equal(sess.read_live()[alive], orc.read_live()[0][alive], err_msg=f"live, tick {t}")
            c, k = sess.frames()
            oc, ok = orc.frames()
            np.testing.assert_array_equal(c[alive], oc[alive])
            np.testing.assert_array_equal(k[alive], ok[alive])
    compare_state(sess, orc, T - 1, alive)
    frames = reported_frames(S, upto)
    assert alive[frames == WRAP - 2].any() and alive[frames == WRAP - 1].any() and alive[64:].all()
    assert sess.counters()[2] == (~alive).sum()
    assert rolled
    sess.close()


# ---------------------------------------------------------------------------- 4. desync detection past the wrap
@pytest.mark.gpu
def test_gpu_desync_detection_past_the_wrap_matches_oracle_every_tick(gpu_available):
    # the body of test_gpu_desync_detection_matches_oracle_every_tick: two peers, interval 10, the
    # state flipped at tick 200 in three sessions.  With input delay 2 and a lag of at most 1 every
    # input arrives before its frame, so no session ever rolls back: every reported frame is
    # confirmed at both peers, which is why exactly the corrupted sessions raise events.  What passes
    # the wrap here is the reports' cells and histories (frames >= 128), not a rollback.
    import torch
    P = 2
    d, lag, interval, t_bad = 2, (0, 1), 10, 200
    inputs, na, nb = networks(S, T, d, lag)
    oa, ob = oracle_peer(MASK_A, S, d, interval), oracle_peer(MASK_B, S, d, interval)
    ga, gb = gpu_peer(MASK_A, S, d, interval), gpu_peer(MASK_B, S, d, interval)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    di = dev(inputs)
    ua, ra, ub, rb = dev(na[0]), dev(na[1]), dev(nb[0]), dev(nb[1])
    bad = [3, 50, 69]
    reports_after_wrap = 0
    for t in range(T):
        if t == t_bad:
            for s in bad:
                oa.corrupt(s, 4 * P, 0x00100000)  # player 0's rotation: the offset persists
                ga.debug_corrupt(s, 4 * P, 0x00100000)
        ga.run_ticks(di[t:t + 1], ua[t:t + 1], ra)
        gb.run_ticks(di[t:t + 1], ub[t:t + 1], rb)
        for g, o, m, net in ((ga, oa, MASK_A, na), (gb, ob, MASK_B, nb)):
            ost, olf, ona, ons = oracle_tick(o, m, inputs, net, t)
            st, lf, nadv, nsave = g.status()
            np.testing.assert_array_equal(st, ost, err_msg=f"status, tick {t}")
            assert (ost == 0).all(), f"tick {t}"
            np.testing.assert_array_equal(lf, olf, err_msg=f"load frame, tick {t}")
            np.testing.assert_array_equal(nadv, ona, err_msg=f"AdvanceFrames, tick {t}")
            np.testing.assert_array_equal(nsave, ons, err_msg=f"SaveGameStates, tick {t}")
            assert (olf == G.NULL_FRAME).all(), f"tick {t}"
        rep_a, rep_b = ga.take_checksum_reports(), gb.take_checksum_reports()
        (fa, ca), (fb, cb) = exchange_oracle(oa, ob)
        for rep, f, c in ((rep_a, fa, ca), (rep_b, fb, cb)):
            gf, gc = dev_reports_as_oracle(rep)
            np.testing.assert_array_equal(gf, f, err_msg=f"report frames, tick {t}")
            np.testing.assert_array_equal(gc[f >= 0], c[f >= 0], err_msg=f"report checksums, tick {t}")
            reports_after_wrap += int((f >= WRAP).sum())
        ga.receive_checksum_reports(1, rep_b)
        gb.receive_checksum_reports(0, rep_a)
        for g, o in ((ga, oa), (gb, ob)):
            gn, gfr, ghd, glo, gro = g.desync_events()
            on, ofr, ohd, olo, oro = o.desync_events(RB_P2P_EVENTS_KEPT)
            for x, y, what in ((gn, on, "counts"), (gfr, ofr, "frames"), (ghd, ohd, "handles"), (glo, olo, "local"),
                               (gro, oro, "remote")):
                np.testing.assert_array_equal(x, y, err_msg=f"desync events {what}, tick {t}")
    for g in (ga, gb):
        n = g.desync_events()[0]
        assert sorted(np.nonzero(n)[0].tolist()) == bad  # exactly the corrupted sessions
        assert g.counters()[2] == 0
        g.close()
    assert reports_after_wrap == 2 * S * len(range(130, T, interval))  # both peers, every interval past the wrap


# ---------------------------------------------------------------------------- 5. packet-fed ticks past the wrap
PACKET_S, PACKET_D = 96, 1
PACKET_CASES = [  # P, mask, rd, W, stride, max_redo, calls
    (2, 0b01, 2, 8, 32, 2, "live"),
    (2, 0b01, 2, 8, 32, 2, "q"),
    (2, 0b01, 2, 8, 32, 2, "cells"),
    # long re-send windows: a packet's reference input, frame start - 1, lies up to 28 frames back,
    # on the other side of the wrap
    (2, 0b01, 1, 15, 64, 28, "live-140-then-30"),
]


@functools.lru_cache(maxsize=None)
def packet_schedule(P, mask, rd, W_, stride, max_redo):
    """One case's network, its packets (encoded on the device) and the oracle's host-side decode of
    them, made once and only read by the launch plans that share it."""
    import torch

    from ggrs_amd import _lib as L
    inputs, upto, rin = synth_network(PACKET_S, P, T, mask, rd, 1, 5)
    dr = torch.from_numpy(rin).cuda()
    pk, ln, st = _encode_schedule(L.load(), P, PACKET_S, T, mask, rd, upto, dr, stride, seed=11 + P, max_redo=max_redo)
    uptos, recvs, codes = _oracle_packet_deliveries(P, PACKET_S, T, mask, W_, rin.shape[0], pk, ln, st)
    for a in (inputs, upto, uptos, codes):
        a.setflags(write=False)
    return inputs, upto, pk, ln, st, uptos, recvs, codes


@pytest.mark.gpu
@pytest.mark.parametrize("P,mask,rd,W_,stride,max_redo,plan", PACKET_CASES,
                         ids=[f"rd{c[2]}-W{c[3]}-redo{c[5]}-{c[6]}" for c in PACKET_CASES])
def test_gpu_packet_ticks_past_the_wrap_match_oracle(gpu_available, monkeypatch, P, mask, rd, W_, stride, max_redo, plan):
    # built like test_gpu_packet_ticks_match_oracle_p2p
    import torch
    monkeypatch.setenv("RB_P2P_SYNC_TICKS", "0")
    inputs, upto, pk, ln, st, uptos, recvs, codes = packet_schedule(P, mask, rd, W_, stride, max_redo)
    assert (codes >= 0).all()
    remotes = [hh for hh in range(P) if not (mask >> hh) & 1]
    if max_redo > 20:
        assert int(ln.max()) > 32, "the schedule must produce packets past the 32-byte register window"
        # a sender whose receiver already held frames past the wrap (its next new frame, prev + 1, in
        # (128, 128 + 28]) re-sends so far back that the packet's reference input, frame
        # start - 1 = prev - redo, lies before the wrap
        ln_h, st_h = ln.cpu().numpy(), st.cpu().numpy()
        crossing = False
        for hh in remotes:
            nominal = upto[:-1, hh] + 1  # packets of ticks 1 .. T - 1
            crossing |= bool(((ln_h[1:, hh] > 0) & (nominal > WRAP) & (nominal <= WRAP + 28) &
                              (st_h[1:, hh] - 1 < WRAP)).any())
        assert crossing, "no packet's reference input lies across the wrap"
        calls = plan_calls("live", 140) + [(a, min(a + 30, T)) for a in range(140, T, 30)]
    else:
        calls = plan_calls(plan)
    b = (G.SessionBuilder(G.Game.EX_GAME, num_sessions=PACKET_S).with_num_players(P).with_max_prediction_window(W_)
         .with_input_delay(PACKET_D).with_remote_input_delay(rd))
    for hh in range(P):
        b.add_player(PlayerType.Local if (mask >> hh) & 1 else PlayerType.Remote, hh)
    wired = b.start_p2p_session()
    orc = O.OracleP2P(O.EX_GAME, P, W_, PACKET_D, mask, PACKET_S, sparse_saving=False, remote_delay=rd)
    di = torch.from_numpy(inputs.copy()).cuda()
    dstat = torch.zeros((P, PACKET_S), dtype=torch.int32, device="cuda")
    acks = torch.full((P, PACKET_S), -1, dtype=torch.int32, device="cuda")
    rolled = False
    for t0, t1 in calls:
        wired.run_ticks_packets(di[t0:t1], pk[t0:t1], ln[t0:t1], st[t0:t1], dstat, acks)
        for k in range(t0, t1):
            for hh in remotes:
                assert orc.deliver(hh, uptos[k, hh], recvs[k][:, hh, :]) == 0, orc.last_panic()
            for hh in range(P):
                if (mask >> hh) & 1:
                    assert orc.add_local_input(hh, inputs[k, hh]) == 0
            ost, olf, ona, ons = orc.advance()
        t = t1 - 1
        st_, lf, na, ns = wired.status()
        np.testing.assert_array_equal(st_, ost, err_msg=f"status, tick {t}")
        np.testing.assert_array_equal(lf, olf, err_msg=f"LoadGameState frame, tick {t}")
        np.testing.assert_array_equal(na, ona, err_msg=f"AdvanceFrame count, tick {t}")
        np.testing.assert_array_equal(ns, ons, err_msg=f"SaveGameState count, tick {t}")
        np.testing.assert_array_equal(dstat.cpu().numpy()[remotes], codes[t][remotes], err_msg=f"decode, tick {t}")
        np.testing.assert_array_equal(acks.cpu().numpy()[remotes], uptos[t][remotes], err_msg=f"acks, tick {t}")
        rolled |= t >= WRAP and bool((lf != G.NULL_FRAME).any())
        if wants_state(t0, t1):
            compare_state(wired, orc, t)
    assert wired.counters()[2] == 0 and rolled
    wired.close()


# ---------------------------------------------------------------------------- 6. spectators fed past the wrap
@pytest.mark.gpu
def test_gpu_host_feeds_spectators_past_the_wrap(gpu_available):
    """test_gpu_host_feeds_spectators_end_to_end's shape over 300 ticks with host calls of 13 ticks:
    the export windows of rb_p2p_export_confirmed_inputs straddle frames 128 and 256 (its
    `next & 127`).  After every call the spectators' state is the truth's cell of their frame (an
    oracle run with every input delivered ahead) and, where the host still holds that frame's
    confirmed cell, the host's.  Session s is fed s % 4 frames short of the export, so that its
    frame is one the host has confirmed."""
    import torch

    import test_spectator as TS
    game, P, mask, chunk = G.Game.EX_GAME, 2, 0b01, 13
    inputs, upto, rin = TS.host_network(game, P, mask, S, T + 8)
    host = TS.start_host(game, P, mask, S)
    spec = TS.start_spectators(game, P, S)
    di, du, dr = (torch.from_numpy(a).cuda() for a in (inputs, upto, rin))
    feed = TS.Feed(host, T + TS.DELAY + 4)
    seen = TS.host_truth(game, P, mask, inputs, rin, T + 8)
    short = torch.from_numpy((np.arange(S) % 4).astype(np.int32)).cuda()
    compared_host = 0
    rolled = False
    prev = np.full(S, G.NULL_FRAME, np.int32)
    for t0 in range(0, T, chunk):
        t1 = min(t0 + chunk, T)
        host.run_ticks(di[t0:t1], du[t0:t1], dr)
        rolled |= t1 - 1 >= WRAP and bool((host.status()[1] != G.NULL_FRAME).any())
        host.export_confirmed_inputs(feed.inputs, feed.upto, feed.last, feed.disc)
        spec.receive_host_status(feed.last.clone(), feed.disc.clone())
        target = torch.clamp(feed.upto - short, min=G.NULL_FRAME)
        spec.run_ticks(target[None].expand(t1 - t0, S).contiguous(), feed.inputs)
        TS.assert_state_is_truth(spec, seen, f"tick {t1 - 1}")
        cur, recv = spec.frames()
        if t1 - t0 == chunk:  # 13 ticks at catch-up speed 3 reach the newest frame fed (the last call has one tick)
            np.testing.assert_array_equal(cur, target.cpu().numpy(), err_msg=f"tick {t1 - 1}: the spectators caught up")
        assert (cur >= prev).all() and (cur <= target.cpu().numpy()).all()
        prev = cur
        img, cs = spec.read_live()
        tags, himg, hcs = host.read_cells()
        _, conf = host.frames()
        for s in range(S):  # the host's own cell of frame current + 1, once confirmed: another kernel, the same bits
            f = int(cur[s]) + 1
            w = f % TS.W_
            if tags[w, s] == f and f <= conf[s]:
                assert np.array_equal(img[s], himg[w, s]) and np.array_equal(cs[s], hcs[w, s]), f"tick {t1 - 1} session {s}"
                compared_host += 1
    assert (host.export_status()[0] == TS.L.RB_P2P_EXPORT_OK).all()
    assert prev.min() > 2 * WRAP and compared_host > S
    adv, thr, far = spec.totals()
    assert adv == int((prev + 1).sum()) and far == 0
    assert host.counters()[2] == 0 and rolled
    host.close()
    spec.close()
