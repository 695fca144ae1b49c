"""Batched time sync of P2P batches: frames_ahead, WaitRecommendation and the
per-endpoint frame advantages (time_sync.rs; protocol.rs:268-277, 439-455,
697-708; p2p_session.rs:318-323, 387-392, 745-776).

The oracle library has no time sync, so this file carries its own restatement
of the reference's code (TimeSync, update_local_frame_advantage,
max_frame_advantage, check_wait_recommendation), line for line, with the
average in numpy.float32.  Everything is integer-exact: every comparison is
equality.
"""
import ctypes

import numpy as np
import pytest

import ggrs_amd as G
from ggrs_amd import _lib as L
from ggrs_amd.p2p import PlayerType, synth_network
from ggrs_amd.session import InvalidRequest
from oracle import oracle as O

NULL_FRAME = -1
FRAME_WINDOW_SIZE = 30       # time_sync.rs:3
RECOMMENDATION_INTERVAL = 60  # p2p_session.rs:23
MIN_RECOMMENDATION = 3        # p2p_session.rs:24
EVENTS_KEPT = L.RB_P2P_WAIT_EVENTS_KEPT
OK, THRESHOLD = 0, 1
F32 = np.float32


# ---------------------------------------------------------------------------
# the reference, restated
# ---------------------------------------------------------------------------
class TimeSync:  # time_sync.rs:6-40
    def __init__(self):
        self.local = [0] * FRAME_WINDOW_SIZE
        self.remote = [0] * FRAME_WINDOW_SIZE

    def advance_frame(self, frame, local_adv, remote_adv):  # :25-28
        self.local[frame % len(self.local)] = local_adv
        self.remote[frame % len(self.remote)] = remote_adv

    def average_frame_advantage(self):  # :30-39
        local_sum = sum(self.local)
        local_avg = F32(local_sum) / F32(len(self.local))
        remote_sum = sum(self.remote)
        remote_avg = F32(remote_sum) / F32(len(self.remote))
        return int((remote_avg - local_avg) / F32(2.0))  # `as i32`: towards zero


def quotient_of_sums(local_sums, remote_sums):
    """average_frame_advantage's f32 value before the cast, over arrays of window sums."""
    la = np.asarray(local_sums, np.int32).astype(F32) / F32(FRAME_WINDOW_SIZE)
    ra = np.asarray(remote_sums, np.int32).astype(F32) / F32(FRAME_WINDOW_SIZE)
    return (ra - la) / F32(2.0)


def average_of_sums(local_sums, remote_sums):
    return quotient_of_sums(local_sums, remote_sums).astype(np.int32)  # astype truncates towards zero


def c_div(a, b):
    """i32 division as Rust's `/` (towards zero)."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


class Endpoint:  # the time-sync fields of UdpProtocol (protocol.rs:118-160)
    def __init__(self, fps):
        self.fps = fps
        self.time_sync_layer = TimeSync()
        self.local_frame_advantage = 0
        self.remote_frame_advantage = 0
        self.round_trip_time = 0

    def update_local_frame_advantage(self, local_frame, last_recv_frame):  # protocol.rs:268-277
        if local_frame == NULL_FRAME or last_recv_frame == NULL_FRAME:
            return
        ping = c_div(self.round_trip_time, 2)
        remote_frame = last_recv_frame + c_div(ping * self.fps, 1000)
        self.local_frame_advantage = remote_frame - local_frame

    def average_frame_advantage(self):  # protocol.rs:314-316
        return self.time_sync_layer.average_frame_advantage()

    def send_input(self, frame):  # protocol.rs:439-455 (frame = the local input's frame)
        self.time_sync_layer.advance_frame(frame, self.local_frame_advantage, self.remote_frame_advantage)


class SessionModel:
    """One P2PSession's time sync, driven by what each advance_frame knows."""

    def __init__(self, P, local_mask, input_delay, fps):
        self.remotes = {h: Endpoint(fps) for h in range(P) if not (local_mask >> h) & 1}
        self.input_delay = input_delay
        self.frames_ahead = 0           # p2p_session.rs:199
        self.next_recommended_sleep = 0  # :198
        self.events = []                # (current_frame, skip_frames)
        self.dead = False

    def max_frame_advantage(self, disconnected):  # :745-761
        interval = None
        for h, ep in self.remotes.items():
            if not disconnected[h]:
                a = ep.average_frame_advantage()
                interval = a if interval is None else max(interval, a)
        return 0 if interval is None else interval

    def advance_frame(self, cur, status, disc_entry, disc_after, last_recv):
        """cur: current_frame at entry; status: Ok / PredictionThreshold / anything else = panic;
        disc_entry / disc_after [P]: local_connect_status[h].disconnected at the tick's entry and
        after update_player_disconnects; last_recv [P]: each endpoint's last_recv_frame after the poll."""
        if self.dead:
            return
        for h, ep in self.remotes.items():  # poll_remote_clients, :387-392
            if not disc_entry[h]:  # is_running()
                ep.update_local_frame_advantage(cur, int(last_recv[h]))
        if status not in (OK, THRESHOLD):  # the process aborted
            self.dead = True
            return
        self.frames_ahead = self.max_frame_advantage(disc_after)  # check_wait_recommendation, :763-776
        if cur > self.next_recommended_sleep and self.frames_ahead >= MIN_RECOMMENDATION:
            self.next_recommended_sleep = cur + RECOMMENDATION_INTERVAL
            self.events.append((cur, self.frames_ahead))
        if status == OK:  # add_local_input did not fail (:334): send_input for every running endpoint
            for h, ep in self.remotes.items():
                if not disc_after[h]:
                    ep.send_input(cur + self.input_delay)


class BatchModel:
    def __init__(self, S, P, local_mask, input_delay, fps):
        self.S, self.P, self.mask = S, P, local_mask
        self.sessions = [SessionModel(P, local_mask, input_delay, fps) for _ in range(S)]

    def receive_quality(self, h, rtt=None, adv=None):
        for s, m in enumerate(self.sessions):
            if rtt is not None:
                m.remotes[h].round_trip_time = int(rtt[s])
            if adv is not None:
                m.remotes[h].remote_frame_advantage = int(adv[s])

    def tick(self, cur, status, disc_entry, disc_after, last_recv):
        """cur, status [S]; disc_* [S, P]; last_recv [P, S]"""
        for s, m in enumerate(self.sessions):
            m.advance_frame(int(cur[s]), int(status[s]), disc_entry[s], disc_after[s], last_recv[:, s])

    def state(self):
        """What the batch exposes: frames_ahead [S], local_adv, remote_adv, rtt [P, S], windows
        [2, 30, P, S], event counts [S], frames and skips [S, E]."""
        S, P = self.S, self.P
        fa = np.array([m.frames_ahead for m in self.sessions], np.int32)
        la, ra, rtt = (np.zeros((P, S), np.int32) for _ in range(3))
        win = np.zeros((2, FRAME_WINDOW_SIZE, P, S), np.int32)
        n = np.zeros(S, np.uint32)
        fr = np.full((S, EVENTS_KEPT), NULL_FRAME, np.int32)
        sk = np.zeros((S, EVENTS_KEPT), np.int32)
        for s, m in enumerate(self.sessions):
            for h, ep in m.remotes.items():
                la[h, s], ra[h, s], rtt[h, s] = ep.local_frame_advantage, ep.remote_frame_advantage, ep.round_trip_time
                win[0, :, h, s] = ep.time_sync_layer.local
                win[1, :, h, s] = ep.time_sync_layer.remote
            n[s] = len(m.events)
            for e, (f, k) in enumerate(m.events[-EVENTS_KEPT:]):
                fr[s, e], sk[s, e] = f, k
        return dict(frames_ahead=fa, local_adv=la, remote_adv=ra, rtt=rtt, windows=win, counts=n, ev_frames=fr, ev_skips=sk)


def host_average(local_sums, remote_sums, device=-1):
    l = np.ascontiguousarray(local_sums, np.int32)
    r = np.ascontiguousarray(remote_sums, np.int32)
    out = np.empty(l.size, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.load().rb_debug_time_sync_average(device, p(l), p(r), p(out), l.size) == 0
    return out


# ---------------------------------------------------------------------------
# KATs and the host function
# ---------------------------------------------------------------------------
KATS = [(0, 0, 0), (5, -5, -5), (-1, 1, 1), (-4, 4, 4), (-40, 40, 40)]  # time_sync.rs:51-114


def test_reference_kats_on_the_model_and_the_host_function():
    for local_adv, remote_adv, want in KATS:
        ts = TimeSync()
        for i in range(60):
            ts.advance_frame(i, local_adv, remote_adv)
        assert ts.average_frame_advantage() == want
        assert host_average([sum(ts.local)], [sum(ts.remote)])[0] == want


def average_pairs():
    """(local sums, remote sums): every pair within +-600, 2^20 random pairs within +-3,840 (the i8
    range times 30) and 2^20 within +-2^20."""
    v = np.arange(-600, 601, dtype=np.int32)
    l0, r0 = (a.ravel() for a in np.meshgrid(v, v, indexing="ij"))
    rng = np.random.default_rng(0x7153)
    l1, r1 = rng.integers(-3840, 3841, (2, 1 << 20), dtype=np.int32)
    l2, r2 = rng.integers(-(1 << 20), (1 << 20) + 1, (2, 1 << 20), dtype=np.int32)
    return np.concatenate([l0, l1, l2]), np.concatenate([r0, r1, r2])


def test_host_average_equals_the_model():
    l, r = average_pairs()
    q = quotient_of_sums(l, r)
    assert ((q < 0) & (q != np.floor(q))).sum() > 1000, "pairs where truncation and floor differ must be present"
    want = average_of_sums(l, r)
    assert (want[(q < 0) & (q != np.floor(q))] == np.ceil(q[(q < 0) & (q != np.floor(q))])).all()
    # the vector model is the scalar one
    for i in np.random.default_rng(1).integers(0, l.size, 2000):
        ts = TimeSync()
        ts.local[0], ts.remote[0] = int(l[i]), int(r[i])
        assert ts.average_frame_advantage() == want[i]
    got = host_average(l, r)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (l[bad[:5]], r[bad[:5]], got[bad[:5]], want[bad[:5]])


# ---------------------------------------------------------------------------
# the schedule
# ---------------------------------------------------------------------------
S, W, T, FPS = 70, 8, 210, 60
STALL = (80, 101)  # the stalled class: no deliveries of its first remote handle in ticks [80, 101): 21 > W
EPOCH = 12


def network(P, mask, rd, ticks=T, dtype=np.uint8, imask=0x0F, stall=True, n=S):
    inputs, upto, rin = synth_network(n, P, ticks, mask, rd, 1, 4, dtype=dtype, mask=imask)
    if stall:
        h = [x for x in range(P) if not (mask >> x) & 1][0]
        cls3 = np.arange(n) % 4 == 3
        a, b = STALL
        upto[a:b, h, cls3] = upto[a - 1, h, cls3]
    return inputs, upto, rin


def quality(epoch, h, n=S):
    """(rtt_ms [n], frame_advantage [n]) the endpoint of handle h receives before tick epoch * 12.
    Classes s % 4: balanced, ahead, behind, stalled (balanced values)."""
    s = np.arange(n)
    cls = s % 4
    rtt = np.select([cls == 1, cls == 2], [0, 333 + 2 * (epoch % 3)], 16 * (epoch % 3)).astype(np.int32)
    adv = np.select([cls == 1, cls == 2], [6 + epoch % 2, -6 - epoch % 2], -3 - epoch % 2 + (h & 1)).astype(np.int32)
    return rtt, adv


def last_recv_of(upto_t, remote_frames):
    return np.minimum(upto_t, remote_frames - 1)


T_REP = 70  # the peers' connect-status reports are given before this tick


def peer_reports(t_rep, upto, P, D):
    """The connect-status reports (endpoint, last_frames [P, n], disconnected [P, n]) of both
    endpoints (P = 3, handles 1 and 2 remote) given before tick t_rep, shaped like
    tests/test_p2p_peer_status.py's: every player at the frame we hold after that tick's poll, and
    endpoint 2 reports player 1 disconnected in the even sessions: in sessions s % 4 == 0 at the
    frame we hold, in sessions s % 4 == 2 two frames before it (GGRS re-triggers that disconnect
    every tick until load_frame's assert fires: those sessions panic).  The reports take effect in
    update_player_disconnects of tick t_rep: that tick's poll still sees player 1 connected (entry
    bit clear), its max_frame_advantage and send_input do not (after bit set)."""
    n = upto.shape[2]
    out = []
    for e in (1, 2):
        last = np.full((P, n), -1, np.int32)
        disc = np.zeros((P, n), np.uint8)
        for i in range(1, P):
            last[i] = np.maximum(upto[t_rep, i], -1)
        last[0] = t_rep - 1 + D
        if e == 2:
            disc[1, np.arange(n) % 2 == 0] = 1
            early = np.arange(n) % 4 == 2
            last[1, early] = upto[t_rep, 1, early] - 2
        out.append((e, last, disc))
    return out


PEER = dict(P=3, mask=0b001, D=1, RD=2)


def test_peer_reported_disconnect_schedule_on_the_oracle():
    """The schedule of the GPU's peer-status cases on the oracle: the disconnect tick has entry and
    after bits that differ, and it has sessions that panic (whose time sync must stop there)."""
    P, mask, D, RD = (PEER[k] for k in ("P", "mask", "D", "RD"))
    inputs, upto, rin = network(P, mask, RD)
    orc = O.OracleP2P(O.EX_GAME, P, W, D, mask, S, remote_delay=RD)
    model = BatchModel(S, P, mask, D, FPS)
    panicked_at = np.full(S, -1)
    differ = np.zeros(S, bool)
    for t in range(T):
        if t % EPOCH == 0:
            for h in (1, 2):
                model.receive_quality(h, *quality(t // EPOCH, h))
        if t == T_REP:
            for e, last, disc in peer_reports(T_REP, upto, P, D):
                orc.receive_peer_connect_status(e, last, disc)
        cur = orc.frames()[0].copy()
        d0 = orc.queues()[:, :, 7].copy()
        for h in (1, 2):
            orc.deliver(h, upto[t, h], rin[:, h, :])
        orc.add_local_input(0, inputs[t, 0])
        st = orc.advance()[0]
        d1 = orc.queues()[:, :, 7]
        panicked_at[(st == O.KIND_PANIC) & (panicked_at < 0)] = t
        if t == T_REP:
            differ = (d0[:, 1] == 0) & (d1[:, 1] == 1)
        frozen = model.state()
        model.tick(cur, st, d0, d1, last_recv_of(upto[t], rin.shape[0]))
        now = model.state()
        dead = (panicked_at >= 0) & (panicked_at < t)
        for k in now:  # a session that panicked stays as its last tick left it
            a, b = (now[k][dead], frozen[k][dead]) if k in ("counts", "ev_frames", "ev_skips") else \
                (now[k][..., dead], frozen[k][..., dead])
            np.testing.assert_array_equal(a, b)
    even = np.arange(S) % 2 == 0
    assert differ[even].sum() >= 8 and not differ[~even].any()
    assert (panicked_at[np.arange(S) % 4 == 2] >= T_REP).all(), "the early report must panic its sessions"
    survived = even & (panicked_at < 0)
    assert survived.sum() >= 4 and (panicked_at[~even] < 0).all()
    orc.close()


def test_schedule_on_the_oracle_shows_every_class():
    P, mask, D, RD = 2, 0b01, 0, 0
    inputs, upto, rin = network(P, mask, RD)
    orc = O.OracleP2P(O.EX_GAME, P, W, D, mask, S, remote_delay=RD)
    model = BatchModel(S, P, mask, D, FPS)
    cls = np.arange(S) % 4
    fa_hist, st_hist, win_moved, ra_hist = [], [], [], []
    trunc_seen = np.zeros(S, bool)
    for t in range(T):
        if t % EPOCH == 0:
            model.receive_quality(1, *quality(t // EPOCH, 1))
        cur = orc.frames()[0].copy()
        d0 = orc.queues()[:, :, 7].copy()
        orc.deliver(1, upto[t, 1], rin[:, 1, :])
        orc.add_local_input(0, inputs[t, 0])
        st = orc.advance()[0]
        assert (st != O.KIND_PANIC).all()
        before = model.state()["windows"]
        model.tick(cur, st, d0, orc.queues()[:, :, 7], last_recv_of(upto[t], rin.shape[0]))
        now = model.state()
        fa_hist.append(now["frames_ahead"])
        st_hist.append(st.copy())
        ra_hist.append(now["remote_adv"][1])
        win_moved.append((before != now["windows"]).any(axis=(0, 1, 2)))
        # frames_ahead comes from the windows as the tick found them (one remote player, connected)
        q = quotient_of_sums(before[0, :, 1].sum(0), before[1, :, 1].sum(0))
        np.testing.assert_array_equal(now["frames_ahead"], q.astype(np.int32), err_msg=f"tick {t}")
        trunc_seen |= (now["frames_ahead"] < 0) & (q != np.floor(q))
    fa_hist, st_hist, win_moved, ra_hist = (np.array(x) for x in (fa_hist, st_hist, win_moved, ra_hist))
    end = model.state()
    # balanced and stalled: no event, ever
    assert (end["counts"][(cls == 0) | (cls == 3)] == 0).all()
    # ahead: at least two events per session, more than 60 frames apart
    for s in np.nonzero(cls == 1)[0]:
        ev = model.sessions[s].events
        assert len(ev) >= 2 and all(b[0] - a[0] > 60 for a, b in zip(ev, ev[1:])) and all(k >= 3 for _, k in ev)
    # behind: negative frames_ahead from a truncated (not floored) average, and no event
    behind = cls == 2
    assert (end["frames_ahead"][behind] < 0).all() and trunc_seen[behind].all() and (end["counts"][behind] == 0).all()
    # stalled: PredictionThreshold ticks; on them the windows stay while frames_ahead is still recomputed
    thr = st_hist == THRESHOLD
    assert thr[:, cls == 3].any(axis=0).all() and not thr[:, cls != 3].any()
    assert not win_moved[thr].any()
    assert win_moved[(st_hist == OK) & (np.arange(T)[:, None] >= 40)].any()
    # frames_ahead is recomputed on those ticks from windows that stand still: a quality report that
    # lands inside the stall (tick 96) changes remote_frame_advantage and must not move frames_ahead,
    # which from a session's second threshold tick on stays what the tick before computed
    held = thr[1:] & thr[:-1]
    assert (held & (ra_hist[1:] != ra_hist[:-1])).any(axis=0)[cls == 3].all(), "a quality change must land in every stall"
    assert (fa_hist[1:][held] == fa_hist[:-1][held]).all()
    orc.close()


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def make_session(game, P, mask, D, RD, sparse=False, desync=0, peer=False, fanout=False, sessions=S, fps=FPS,
                 time_sync=True):
    b = (G.SessionBuilder(game, num_sessions=sessions).with_num_players(P).with_max_prediction_window(W)
         .with_input_delay(D).with_remote_input_delay(RD).with_sparse_saving_mode(sparse).with_block_size(256))
    if desync:
        b.with_desync_detection_mode(desync)
    if peer:
        b.with_peer_connect_status(True)
    if fanout:
        b.with_speculative_fanout(True, adaptive=False)
    for h in range(P):
        b.add_player(PlayerType.Local if (mask >> h) & 1 else PlayerType.Remote, h)
    sess = b.start_p2p_session()
    if time_sync:
        sess.enable_time_sync(fps)
    return sess


def gpu_state(sess):
    fa, la, ra, rtt = sess.read_time_sync()
    n, fr, sk = sess.wait_recommendations()
    return dict(frames_ahead=fa, local_adv=la, remote_adv=ra, rtt=rtt, windows=sess.debug_time_sync_windows(),
                counts=n, ev_frames=fr, ev_skips=sk)


def assert_same(got, want, what, rows=None):
    for k in want:
        a, b = got[k], want[k]
        if rows is not None:  # sessions to compare (the last axis, or the first for the event arrays)
            a, b = (a[rows], b[rows]) if k in ("counts", "ev_frames", "ev_skips") else (a[..., rows], b[..., rows])
        np.testing.assert_array_equal(a, b, err_msg=f"{k}, {what}")


def send_quality(sess, model, epoch, remotes):
    import torch
    for h in remotes:
        rtt, adv = quality(epoch, h, sess.num_sessions)
        sess.receive_quality(h, torch.from_numpy(rtt).cuda(), torch.from_numpy(adv).cuda())
        if model is not None:
            model.receive_quality(h, rtt, adv)


EVERY_TICK = {
    "stub_p2": dict(game=G.Game.STUB, P=2, mask=0b01, D=0, RD=0, fps=60, dtype=np.uint32, imask=0x3),
    "exgame_p2": dict(game=G.Game.EX_GAME, P=2, mask=0b01, D=0, RD=1, fps=60),
    "exgame_p4": dict(game=G.Game.EX_GAME, P=4, mask=0b0011, D=2, RD=1, fps=50),
    "exgame_p3_disconnect": dict(game=G.Game.EX_GAME, P=3, mask=0b001, D=1, RD=0, fps=60, disconnect=(90, 1)),
    # peers' connect-status reports before tick 70: on that tick the poll sees player 1 connected and
    # send_input does not (kTlEntry against kTlEnd); some of its sessions panic, on that tick or later
    "exgame_p3_peer_status": dict(game=G.Game.EX_GAME, fps=60, peer=True, desync=10, **PEER),
    # the orbit test game through the plug-in path: the logging P2P kernels of the plug-in's own library
    "orbit_plugin_p3": dict(game="orbit", P=3, mask=0b010, D=1, RD=1, fps=60, imask=0x1F),
}


def game_of(c):
    if c["game"] != "orbit":
        return c["game"]
    import os
    from ggrs_amd.plugin import register_game_plugin
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return register_game_plugin(os.path.join(root, "tests", "plugin_game", "libggrs_game_orbit.so"))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(EVERY_TICK))
def test_gpu_every_tick_against_the_model(gpu_available, case):
    import torch
    c = EVERY_TICK[case]
    P, mask, D = c["P"], c["mask"], c["D"]
    remotes = [h for h in range(P) if not (mask >> h) & 1]
    inputs, upto, rin = network(P, mask, c["RD"], dtype=c.get("dtype", np.uint8), imask=c.get("imask", 0x0F))
    sess = make_session(game_of(c), P, mask, D, c["RD"], fps=c["fps"], peer=c.get("peer", False),
                        desync=c.get("desync", 0))
    model = BatchModel(S, P, mask, D, c["fps"])
    panicked_at = np.full(S, -1)
    di, du, dr = (torch.from_numpy(a).cuda() for a in (inputs, upto, rin))
    half = np.arange(S) % 2 == 0
    frozen = None
    for t in range(T):
        if t % EPOCH == 0:
            send_quality(sess, model, t // EPOCH, remotes)
        if c.get("disconnect") and t == c["disconnect"][0]:
            sess.disconnect_player(c["disconnect"][1], half)
            frozen = gpu_state(sess)["windows"][:, :, c["disconnect"][1]][..., half].copy()
        if c.get("peer") and t == T_REP:
            for e, last, disc in peer_reports(T_REP, upto, P, D):
                sess.receive_peer_connect_status(e, torch.from_numpy(last).cuda(), torch.from_numpy(disc).cuda())
        cur = sess.frames()[0]
        d0 = sess.read_queues()[:, :, 7]
        if t == T - 1:
            last_win = gpu_state(sess)["windows"]
        sess.run_ticks(di[t:t + 1], du[t:t + 1], dr)
        st = sess.status()[0]
        if not c.get("peer"):
            assert ((st == OK) | (st == THRESHOLD)).all(), f"tick {t}: {st}"
        panicked_at[(st == L.RB_PANIC) & (panicked_at < 0)] = t
        d1 = sess.read_queues()[:, :, 7]
        if c.get("peer") and t == T_REP:
            differ = (d0[:, 1] == 0) & (d1[:, 1] == 1)
        # (a panicked session: the model applies the poll of the tick that panicked and stops there)
        model.tick(cur, st, d0, d1, last_recv_of(upto[t], rin.shape[0]))
        assert_same(gpu_state(sess), model.state(), f"{case}, tick {t}")
    end = gpu_state(sess)
    if c.get("peer"):
        even = np.arange(S) % 2 == 0
        assert differ[even].sum() >= 8 and (panicked_at[np.arange(S) % 4 == 2] >= T_REP).all()
        assert (even & (panicked_at < 0)).sum() >= 4
    else:
        assert (end["counts"][np.arange(S) % 4 == 1] >= 2).all()
    if c.get("disconnect"):
        h = c["disconnect"][1]
        np.testing.assert_array_equal(end["windows"][:, :, h][..., half], frozen)  # the endpoint stopped
        other = [x for x in remotes if x != h][0]
        lsum, rsum = last_win[0, :, other].sum(0), last_win[1, :, other].sum(0)  # as the last tick found them
        np.testing.assert_array_equal(end["frames_ahead"][half], average_of_sums(lsum, rsum)[half])  # out of the maximum
    sess.close()


@pytest.mark.gpu
def test_gpu_session_whose_only_remote_player_is_gone_reports_zero(gpu_available):
    import torch
    P, mask = 2, 0b01
    inputs, upto, rin = network(P, mask, 0, ticks=60, stall=False)
    sess = make_session(G.Game.EX_GAME, P, mask, 0, 0)
    di, du, dr = (torch.from_numpy(a).cuda() for a in (inputs, upto, rin))
    send_quality(sess, None, 0, [1])
    sess.run_ticks(di[:40], du[:40], dr)
    assert (sess.frames_ahead()[np.arange(S) % 4 == 1] >= 3).all()
    half = np.arange(S) % 2 == 0
    sess.disconnect_player(1, half)
    before = gpu_state(sess)
    sess.run_ticks(di[40:60], du[40:60], dr)
    after = gpu_state(sess)
    assert (sess.status()[0] == OK).all()
    assert (after["frames_ahead"][half] == 0).all()
    np.testing.assert_array_equal(after["windows"][..., half], before["windows"][..., half])
    np.testing.assert_array_equal(after["counts"][half], before["counts"][half])
    assert (after["frames_ahead"][~half & (np.arange(S) % 4 == 1)] >= 3).all()
    sess.close()


def run_in_launches(sess, di, du, dr, bounds, plan, remotes, reports=None):
    """Ticks [0, bounds[-1]) in launches of at most `plan` ticks cut at `bounds`, quality values
    sent at every bound; the time-sync state at every bound."""
    out = []
    for k, (a, b) in enumerate(zip(bounds, bounds[1:])):
        send_quality(sess, None, k, remotes)
        if reports and k in reports:
            reports[k](sess)
        for t in range(a, b, plan):
            e = min(t + plan, b)
            sess.run_ticks(di[t:e], du[t:e], dr)
        out.append(gpu_state(sess))
    return out


FUSED = {
    "plain": dict(game=G.Game.EX_GAME, P=2, mask=0b01, D=1, RD=1),
    "sparse": dict(game=G.Game.EX_GAME, P=2, mask=0b01, D=1, RD=1, sparse=True),
    "desync_peer": dict(game=G.Game.EX_GAME, desync=10, peer=True, **PEER),
    "fanout_inkernel": dict(game=G.Game.EX_GAME, P=2, mask=0b01, D=1, RD=1, fanout=True),
    "fanout_two_launch": dict(game=G.Game.BRAWLER, P=2, mask=0b01, D=1, RD=1, fanout=True, sessions=6),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(FUSED))
def test_gpu_fused_launches_equal_one_tick_launches(gpu_available, case):
    import torch
    c = FUSED[case]
    P, mask = c["P"], c["mask"]
    remotes = [h for h in range(P) if not (mask >> h) & 1]
    bounds = [0, 70, 140, 210]  # shared by the plans of 1, 7 and 50 (50 + 20) ticks
    n = c.get("sessions", S)
    inputs, upto, rin = network(P, mask, c["RD"], n=n)
    di, du, dr = (torch.from_numpy(a).cuda() for a in (inputs, upto, rin))
    # the peers' reports given at bound 1 land in the first tick of the 50-tick launch: the poll of
    # that tick still sees the player connected (entry bit), send_input does not; some of those
    # sessions panic, on that tick or on a later tick of the launch
    reports = None
    if c.get("peer"):
        def give(sess):
            for e, last, disc in peer_reports(T_REP, upto, P, c["D"]):
                sess.receive_peer_connect_status(e, torch.from_numpy(last).cuda(), torch.from_numpy(disc).cuda())
        assert bounds[1] == T_REP
        reports = {1: give}
    res = {}
    for plan in (1, 7, 50):
        sess = make_session(c["game"], P, mask, c["D"], c["RD"], sparse=c.get("sparse", False),
                            desync=c.get("desync", 0), peer=c.get("peer", False), fanout=c.get("fanout", False),
                            sessions=n)
        res[plan] = run_in_launches(sess, di, du, dr, bounds, plan, remotes, reports)
        res[plan, "status"] = sess.status()[0]
        res[plan, "queues"] = sess.read_queues()
        sess.close()
    np.testing.assert_array_equal(res[7, "status"], res[1, "status"])
    np.testing.assert_array_equal(res[50, "status"], res[1, "status"])
    for plan in (7, 50):  # every session, the panicked ones included: their time sync stopped at the same tick
        for k in range(len(bounds) - 1):
            assert_same(res[plan][k], res[1][k], f"{case}: launches of {plan} against 1, bound {bounds[k + 1]}")
    assert (res[1][-1]["windows"] != 0).any()
    if c.get("peer"):
        panicked = res[1, "status"] == L.RB_PANIC
        even = np.arange(n) % 2 == 0
        assert panicked[np.arange(n) % 4 == 2].all() and not panicked[~even].any()
        assert (even & ~panicked).sum() >= 4 and (res[1, "queues"][even & ~panicked][:, 1, 7] == 1).all()


@pytest.mark.gpu
def test_gpu_time_sync_moves_nothing_else(gpu_available):
    import torch
    P, mask, D, RD = 2, 0b01, 1, 1
    inputs, upto, rin = network(P, mask, RD)
    di, du, dr = (torch.from_numpy(a).cuda() for a in (inputs, upto, rin))
    out = []
    for on in (True, False):
        sess = make_session(G.Game.EX_GAME, P, mask, D, RD, time_sync=on)
        if on:
            send_quality(sess, None, 0, [1])
        for a, b in ((0, 50), (50, 57), (57, 58), (58, 108), (108, T)):
            sess.run_ticks(di[a:b], du[a:b], dr)
        out.append((sess.read_cells(), sess.read_live(), sess.frames(), sess.read_queues(), sess.status()))
        sess.close()
    for x, y in zip(*out):
        for a, b in zip(x, y) if isinstance(x, tuple) else ((x, y),):
            np.testing.assert_array_equal(a, b)


@pytest.mark.gpu
def test_gpu_device_average_equals_the_host(gpu_available):
    l, r = average_pairs()
    np.testing.assert_array_equal(host_average(l, r, device=0), host_average(l, r))


@pytest.mark.gpu
def test_gpu_export_equals_read(gpu_available):
    import torch
    P, mask = 3, 0b001
    inputs, upto, rin = network(P, mask, 1, ticks=60, stall=False)
    sess = make_session(G.Game.EX_GAME, P, mask, 1, 1)
    di, du, dr = (torch.from_numpy(a).cuda() for a in (inputs, upto, rin))
    send_quality(sess, None, 0, [1, 2])
    sess.run_ticks(di, du, dr)
    fa = torch.full((S,), 77, dtype=torch.int32, device="cuda")
    la = torch.full((P, S), 77, dtype=torch.int32, device="cuda")
    sess.export_time_sync(fa, la)
    hfa, hla, hra, hrtt = sess.read_time_sync()
    np.testing.assert_array_equal(fa.cpu().numpy(), hfa)
    np.testing.assert_array_equal(la.cpu().numpy(), hla)
    assert (hla[1:] != 0).any() and (hla[0] == 0).all()
    ns = sess.network_stats(2)
    np.testing.assert_array_equal(ns["ping"], hrtt[2])
    np.testing.assert_array_equal(ns["local_frames_behind"], hla[2])
    np.testing.assert_array_equal(ns["remote_frames_behind"], hra[2])
    np.testing.assert_array_equal(sess.frames_ahead(), hfa)
    sess.close()


@pytest.mark.gpu
def test_gpu_validation(gpu_available):
    import torch
    P, mask = 2, 0b01
    inputs, upto, rin = network(P, mask, 0, ticks=4, stall=False)
    di, du, dr = (torch.from_numpy(a).cuda() for a in (inputs, upto, rin))
    z = torch.zeros(S, dtype=torch.int32, device="cuda")

    def refused(fn, text):
        with pytest.raises(InvalidRequest) as e:
            fn()
        assert text in str(e.value), str(e.value)

    sess = make_session(G.Game.EX_GAME, P, mask, 0, 0, time_sync=False)
    refused(lambda: sess.enable_time_sync(0), "FPS should be higher than 0.")
    refused(lambda: sess.enable_time_sync(-5), "FPS should be higher than 0.")
    for read in (sess.frames_ahead, sess.wait_recommendations, sess.debug_time_sync_windows,
                 lambda: sess.network_stats(1), lambda: sess.receive_quality(1, z, z),
                 lambda: sess.export_time_sync(z, None)):
        refused(read, "time sync is off")
    sess.enable_time_sync(60)  # the refused calls changed nothing: this is still the first enable
    refused(lambda: sess.enable_time_sync(60), "already on")
    refused(lambda: sess.receive_quality(0, z, z), "remote handle")
    refused(lambda: sess.receive_quality(2, z, z), "remote handle")
    refused(lambda: sess.network_stats(0), "Given player handle not referring to a remote player or spectator")
    state = gpu_state(sess)
    assert all((v == 0).all() for k, v in state.items() if k != "ev_frames") and (state["ev_frames"] == NULL_FRAME).all()
    pk = torch.zeros((1, P, S, 32), dtype=torch.uint8, device="cuda")
    n = torch.zeros((1, P, S), dtype=torch.int32, device="cuda")
    refused(lambda: sess.run_ticks_packets(di[:1], pk, n, n), "time sync takes rb_p2p_run_ticks")
    assert (sess.frames()[0] == 0).all()
    sess.close()

    late = make_session(G.Game.EX_GAME, P, mask, 0, 0, time_sync=False)
    late.run_ticks(di[:1], du[:1], dr)
    refused(lambda: late.enable_time_sync(60), "before the batch's first tick")
    refused(late.frames_ahead, "time sync is off")
    late.run_ticks(di[1:2], du[1:2], dr)
    assert (late.frames()[0] == 2).all()
    late.close()


@pytest.mark.gpu
def test_gpu_plugin_built_before_the_tick_log_is_refused_time_sync(gpu_available, tmp_path):
    """A plug-in library without rb_plugin_tick_log (its P2P kernels would never write the log) loads
    and ticks as before, and rb_p2p_time_sync_enable refuses it.  The stand-in is a copy of the
    orbit plug-in whose symbol name is changed in place, so a lookup of the name finds nothing."""
    import os
    import torch
    from ggrs_amd.plugin import register_game_plugin
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    blob = open(os.path.join(root, "tests", "plugin_game", "libggrs_game_orbit.so"), "rb").read()
    assert blob.count(b"rb_plugin_tick_log\0") >= 1
    old = tmp_path / "libggrs_game_orbit_old.so"
    old.write_bytes(blob.replace(b"rb_plugin_tick_log\0", b"rb_plugin_tick_lo_\0"))
    gid = register_game_plugin(str(old))
    assert gid != game_of(dict(game="orbit"))
    P, mask = 3, 0b010
    inputs, upto, rin = network(P, mask, 1, ticks=4, stall=False, imask=0x1F)
    di, du, dr = (torch.from_numpy(a).cuda() for a in (inputs, upto, rin))
    sess = make_session(gid, P, mask, 1, 1, time_sync=False)
    with pytest.raises(InvalidRequest) as e:
        sess.enable_time_sync(60)
    assert "rebuild the game plugin" in str(e.value)
    with pytest.raises(InvalidRequest):
        sess.frames_ahead()
    sess.run_ticks(di, du, dr)
    assert (sess.frames()[0] == 4).all() and (sess.status()[0] == OK).all()
    sess.close()
