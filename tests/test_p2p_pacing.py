"""Per-session pacing of P2P batches (include/ggrs_amd.h rb_p2p_run_ticks_paced,
rb_p2p_pace, rb_p2p_read_pacing): the caller's frame loop
of examples/ex_game/ex_game_p2p.rs:80-122, where poll_remote_clients runs on
every iteration and add_local_input / advance_frame only when a frame is due.

The oracle advances all of its sessions at once, but sessions are independent:
the tests keep one OracleP2P per schedule class (session s of the batch is in
class s % C).  On a tick where a class is parked only deliver() is called on its
oracle (poll_remote_clients; oracle_capi.cpp delivers incrementally from
last_frame + 1), on a running tick deliver, add_local_input and advance.  Every
comparison is equality.
"""
import ctypes
import functools

import numpy as np
import pytest

import ggrs_amd as G
from ggrs_amd import _lib as L
from ggrs_amd.p2p import synth_network
from ggrs_amd.session import InvalidRequest
from oracle import oracle as O
from test_p2p import ORC_GAME
from test_time_sync import BatchModel, assert_same, gpu_state, last_recv_of, make_session, peer_reports, PEER, T_REP

W = 8
S, C, T = 70, 4, 120  # 70 sessions: two waves, one partial


# ---------------------------------------------------------------------------
# the pacer, restated (ex_game_p2p.rs:91-104 in integers, at the nominal frame rate)
# ---------------------------------------------------------------------------
def pace_step(acc, frames_ahead):
    """(acc, run) after one tick."""
    acc += 10
    cost = 11 if frames_ahead > 0 else 10  # fps_delta *= 1.1
    run = acc >= cost
    if run:
        acc -= cost
    return acc, run


def test_pacer_model_runs_10_of_11_while_ahead_and_every_tick_otherwise():
    for fa in (1, 3, 100):
        acc, runs = 0, []
        for _ in range(110):
            acc, r = pace_step(acc, fa)
            runs.append(r)
        assert sum(runs) == 100
        for k in range(0, 110, 11):  # exactly one parked tick in every 11
            assert sum(runs[k:k + 11]) == 10
    for fa in (0, -1, -50):
        acc = 0
        for _ in range(50):
            acc, r = pace_step(acc, fa)
            assert r and acc == 0


def test_pacer_model_accumulator_stays_below_21():
    rng = np.random.default_rng(0x9ACE)
    for _ in range(10_000):
        acc = 0
        for fa in rng.integers(-3, 4, 64):
            acc, r = pace_step(acc, int(fa))
            assert 0 <= acc < 21
            assert r or acc < 11  # at most one frame per tick, and a parked tick leaves less than one frame's cost


# ---------------------------------------------------------------------------
# schedules and the class oracles
# ---------------------------------------------------------------------------
def schedule(ticks=T, seed=0x70AC):
    """run[t, c] of the four classes: never parked; parked every 11th tick; parked on a seeded
    random 30% of ticks; parked for one run of 6 consecutive ticks every 40."""
    t = np.arange(ticks)
    run = np.ones((ticks, C), bool)
    run[:, 1] = t % 11 != 10
    run[:, 2] = np.random.default_rng(seed).random(ticks) >= 0.3
    run[:, 3] = ~((t % 40 >= 20) & (t % 40 < 26))
    return run


def session_mask(run_t, n):
    """The run-mask row [n] uint8 of class flags run_t [classes]."""
    run_t = np.asarray(run_t)
    return run_t[np.arange(n) % len(run_t)].astype(np.uint8)


def network(P, mask, rd, n=S, ticks=T, dtype=np.uint8, imask=0x0F, stall=True):
    """Delivery lags 1-4 (tests/test_p2p.py's), and a stall of the first remote handle in the
    sessions s % 5 == 1 (one in every class) over ticks [60, 75): longer than the prediction window."""
    inputs, upto, rin = synth_network(n, P, ticks, mask, rd, 1, 4, dtype=dtype, mask=imask)
    if stall and ticks > 75:
        h = [x for x in range(P) if not (mask >> x) & 1][0]
        who = np.arange(n) % 5 == 1
        upto[60:75, h, who] = upto[59, h, who]
    return inputs, upto, rin


class Classes:
    """One OracleP2P per schedule class; session s of the batch is session s // classes of class
    s % classes.  Keeps what rb_p2p_read_status reports: every session's last advance_frame."""

    def __init__(self, game, P, d, rd, mask, n, sparse=False, classes=C, desync=0):
        self.P, self.mask, self.n = P, mask, n
        self.cols = [np.arange(c, n, classes) for c in range(classes)]
        self.orcs = [O.OracleP2P(ORC_GAME[game], P, W, d, mask, len(k), sparse_saving=sparse, remote_delay=rd)
                     for k in self.cols]
        if desync:
            for o in self.orcs:
                o.set_desync_detection(desync)
        self.st = np.zeros(n, np.int32)
        self.lf, self.na, self.ns = (np.full(n, -1, np.int32) for _ in range(3))  # no tick yet
        self.dead = np.zeros(n, bool)
        self.poll_panics = 0
        self._rin = (None, {})  # the remote inputs by frame of each (handle, class), contiguous, made once per tensor

    def by_frame(self, rin, h, c):
        if self._rin[0] is not rin:
            self._rin = (rin, {})
        if (h, c) not in self._rin[1]:
            self._rin[1][h, c] = np.ascontiguousarray(rin[:, h][:, self.cols[c]])
        return self._rin[1][h, c]

    def tick(self, t, run_c, inputs, upto, rin):
        for c, (orc, k) in enumerate(zip(self.orcs, self.cols)):
            for h in range(self.P):
                if not (self.mask >> h) & 1:
                    rc = orc.deliver(h, upto[t, h][k], self.by_frame(rin, h, c))
                    if rc and not run_c[c]:
                        # a parked poll fired a reference assert: the schedules that get here deliver
                        # the same frames to every session of the class, so all of them panicked
                        self.poll_panics += int((~self.dead[k]).sum())
                        self.st[k] = L.RB_PANIC
                        self.dead[k] = True
            if not run_c[c]:
                continue
            for h in range(self.P):
                if (self.mask >> h) & 1:
                    orc.add_local_input(h, inputs[t, h][k])
            st, lf, na, ns = orc.advance()
            self.st[k] = np.where(st == O.KIND_PANIC, L.RB_PANIC, st)
            self.lf[k], self.na[k], self.ns[k] = lf, na, ns
            self.dead[k] |= st == O.KIND_PANIC

    def gather(self, parts, axis):
        """The batch-order array of per-class arrays whose `axis` is the class's sessions."""
        shape = list(parts[0].shape)
        shape[axis] = self.n
        out = np.zeros(shape, parts[0].dtype)
        for k, a in zip(self.cols, parts):
            idx = [slice(None)] * out.ndim
            idx[axis] = k
            out[tuple(idx)] = a
        return out

    def cells(self):
        parts = [o.read_cells() for o in self.orcs]
        return tuple(self.gather([p[i] for p in parts], 1) for i in range(3))

    def live(self):
        return self.gather([o.read_live()[0] for o in self.orcs], 0)

    def frames(self):
        parts = [o.frames() for o in self.orcs]
        return tuple(self.gather([p[i] for p in parts], 0) for i in range(2))

    def queues(self):
        return self.gather([o.queues() for o in self.orcs], 0)

    def disconnect(self, h, who):
        for o, k in zip(self.orcs, self.cols):
            if who[k].any():
                assert o.disconnect_player(h, who[k]) == 0

    def close(self):
        for o in self.orcs:
            o.close()


def compare_status(sess, cls, what):
    st, lf, na, ns = sess.status()
    np.testing.assert_array_equal(st, cls.st, err_msg=f"status, {what}")
    a = ~cls.dead
    np.testing.assert_array_equal(lf[a], cls.lf[a], err_msg=f"LoadGameState frame, {what}")
    np.testing.assert_array_equal(na[a], cls.na[a], err_msg=f"AdvanceFrame count, {what}")
    np.testing.assert_array_equal(ns[a], cls.ns[a], err_msg=f"SaveGameState count, {what}")


def compare_all(sess, cls, what):
    """Status, load frame, request counts, every cell's tag, image and checksum, live state, frames
    and all 8 queue fields of every player == the class oracles' (a panicked session is dead)."""
    compare_status(sess, cls, what)
    a = ~cls.dead
    tags, imgs, cs = sess.read_cells()
    otags, oimgs, ocs = cls.cells()
    np.testing.assert_array_equal(tags[:, a], otags[:, a], err_msg=f"cell frames, {what}")
    valid = (otags >= 0) & a[None, :]
    np.testing.assert_array_equal(imgs[valid], oimgs[valid], err_msg=f"cell images, {what}")
    np.testing.assert_array_equal(cs[valid], ocs[valid], err_msg=f"cell checksums, {what}")
    np.testing.assert_array_equal(sess.read_live()[a], cls.live()[a], err_msg=f"live state, {what}")
    for x, y, n in zip(sess.frames(), cls.frames(), ("current", "confirmed")):
        np.testing.assert_array_equal(x[a], y[a], err_msg=f"{n} frame, {what}")
    dq, oq = sess.read_queues(), cls.queues()
    # inputs[tail].frame before a queue's first add: NULL in the reference, 0 on the device
    dq[:, :, 1] = np.where(dq[:, :, 0] < 0, oq[:, :, 1], dq[:, :, 1])
    np.testing.assert_array_equal(dq[a], oq[a], err_msg=f"input queues, {what}")


def snapshot(sess):
    """What a parked tick must leave bit-identical: cells, live state, frames, the status and trace words."""
    return sess.read_cells() + (sess.read_live(),) + sess.frames() + sess.status()


def assert_frozen(before, after, who, what):
    for i, (x, y) in enumerate(zip(before, after)):
        ax = 1 if i < 3 else 0
        np.testing.assert_array_equal(np.compress(who, x, ax), np.compress(who, y, ax), err_msg=f"part {i} moved, {what}")


def dev(*arrays):
    import torch
    out = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)
    return out if len(out) > 1 else out[0]


# ---------------------------------------------------------------------------
# the closed loop: time sync -> pacer -> run mask -> paced tick (CPU)
# ---------------------------------------------------------------------------
LOOP = dict(n=70, ticks=160, P=2, mask=0b01, D=0, RD=0, fps=60)


def loop_quality(n):
    """rtt 0 and the peer's frame advantage: balanced (even sessions) -4, ahead (odd) +6.  With
    lags 1-4 a session in step holds local advantages of -5..-2: the balanced average difference
    stays in [-1, 0.5] (frames_ahead 0 or -1), the ahead one starts near +4."""
    return np.zeros(n, np.int32), np.where(np.arange(n) % 2 == 1, 6, -4).astype(np.int32)


def parked_poll(m, cur, disc_entry, last_recv):
    """A parked tick of SessionModel m: poll_remote_clients' update_local_frame_advantage only."""
    if m.dead:
        return
    for h, ep in m.remotes.items():
        if not disc_entry[h]:
            ep.update_local_frame_advantage(cur, int(last_recv[h]))


@functools.lru_cache(maxsize=None)
def closed_loop_reference():
    """The loop on one oracle per session + the time-sync model + the pacer model.  Returns the
    masks [ticks, n], the class oracles (final state) and the model."""
    c = LOOP
    n, ticks, P, mask = c["n"], c["ticks"], c["P"], c["mask"]
    inputs, upto, rin = network(P, mask, c["RD"], n=n, ticks=ticks, stall=False)
    cls = Classes(G.Game.EX_GAME, P, c["D"], c["RD"], mask, n, classes=n)
    model = BatchModel(n, P, mask, c["D"], c["fps"])
    model.receive_quality(1, *loop_quality(n))
    acc = np.zeros(n, np.int64)
    run = np.ones(n, bool)
    masks = np.zeros((ticks, n), np.uint8)
    for t in range(ticks):
        masks[t] = run
        cur = cls.frames()[0]
        d0 = cls.queues()[:, :, 7]
        cls.tick(t, run, inputs, upto, rin)
        d1 = cls.queues()[:, :, 7]
        lr = last_recv_of(upto[t], rin.shape[0])
        for s, m in enumerate(model.sessions):
            if run[s]:
                m.advance_frame(int(cur[s]), int(cls.st[s]), d0[s], d1[s], lr[:, s])
            else:
                parked_poll(m, int(cur[s]), d0[s], lr[:, s])
        fa = model.state()["frames_ahead"]
        for s in range(n):
            acc[s], run[s] = pace_step(int(acc[s]), int(fa[s]))
    return masks, cls, model, (inputs, upto, rin)


def test_closed_loop_parks_the_ahead_class_and_never_the_balanced_one():
    masks, cls, model, _ = closed_loop_reference()
    parked = (masks == 0).sum(0)
    odd = np.arange(LOOP["n"]) % 2 == 1
    assert (parked[odd] >= 1).all(), "every session that is ahead parks at least once"
    assert (parked[~odd] == 0).all(), "a balanced session never parks"
    assert not cls.dead.any() and (cls.st == 0).all()
    cur = cls.frames()[0]
    np.testing.assert_array_equal(cur, LOOP["ticks"] - parked)  # a parked tick is a frame not advanced


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
PARITY = {  # game, P, local mask, input delay, remote delay, sparse, sessions
    "stub-h0-d0": (G.Game.STUB, 2, 0b01, 0, 0, False, S),
    "stub-h1-d2-sparse": (G.Game.STUB, 2, 0b10, 2, 1, True, S),
    "exgame-p2-h0-d0": (G.Game.EX_GAME, 2, 0b01, 0, 0, False, S),
    "exgame-p2-h1-d2-sparse": (G.Game.EX_GAME, 2, 0b10, 2, 1, True, S),
    "exgame-p3-h1-d0-sparse": (G.Game.EX_GAME, 3, 0b010, 0, 1, True, S),
    "exgame-p3-h0-d2": (G.Game.EX_GAME, 3, 0b001, 2, 0, False, S),
    "exgame-p4-h0-d2": (G.Game.EX_GAME, 4, 0b0001, 2, 1, False, S),
    "exgame-p4-h01-d0-sparse": (G.Game.EX_GAME, 4, 0b0011, 0, 0, True, S),
    "brawler-h0-d2": (G.Game.BRAWLER, 2, 0b01, 2, 1, False, 5),
    "brawler-h1-d0-sparse": (G.Game.BRAWLER, 2, 0b10, 0, 0, True, 5),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(PARITY))
def test_gpu_paced_ticks_match_the_class_oracles_every_tick(gpu_available, case):
    game, P, mask, d, rd, sparse, n = PARITY[case]
    stub = game == G.Game.STUB
    inputs, upto, rin = network(P, mask, rd, n=n, dtype=np.uint32 if stub else np.uint8, imask=0x3 if stub else 0x0F)
    run = schedule()
    sess = make_session(game, P, mask, d, rd, sparse=sparse, sessions=n, time_sync=False)
    cls = Classes(game, P, d, rd, mask, n, sparse=sparse)
    di, du, dr = dev(inputs, upto, rin)
    masks = dev(np.stack([session_mask(r, n) for r in run]))
    saw_load = saw_threshold = False
    totals = sess.totals()
    for t in range(T):
        before = snapshot(sess)
        q0 = sess.read_queues()
        sess.run_ticks(di[t:t + 1], du[t:t + 1], dr, run_mask=masks[t:t + 1])
        cls.tick(t, run[t], inputs, upto, rin)
        compare_all(sess, cls, f"{case}, tick {t}")
        parked = session_mask(run[t], n) == 0
        assert_frozen(before, snapshot(sess), parked, f"{case}, tick {t}")
        if not run[t].any():
            assert sess.totals() == totals
        totals = sess.totals()
        q1 = sess.read_queues()  # only the remote queues of a parked session move
        for h in range(P):
            if (mask >> h) & 1:
                np.testing.assert_array_equal(q0[parked, h], q1[parked, h])
        saw_load |= bool((cls.lf[~parked] >= 0).any())
        saw_threshold |= bool((cls.st == 1).any())
    assert saw_load and saw_threshold and not cls.dead.any()
    assert sess.counters()[2] == 0
    np.testing.assert_array_equal(sess.parked_ticks(), (~run).sum(0)[np.arange(n) % C])
    sess.close()
    cls.close()


@pytest.mark.gpu
def test_gpu_a_tick_with_every_session_parked_moves_only_the_remote_queues(gpu_available):
    P, mask, d, rd = 2, 0b01, 1, 1
    inputs, upto, rin = network(P, mask, rd, ticks=40, stall=False)
    di, du, dr = dev(inputs, upto, rin)
    sess = make_session(G.Game.EX_GAME, P, mask, d, rd, time_sync=False)
    sess.run_ticks(di[:20], du[:20], dr)
    before, totals, counters, q0 = snapshot(sess), sess.totals(), sess.counters(), sess.read_queues()
    zeros = dev(np.zeros((3, S), np.uint8))
    sess.run_ticks(di[20:23], du[20:23], dr, run_mask=zeros)
    assert_frozen(before, snapshot(sess), np.ones(S, bool), "three parked ticks")
    assert sess.totals() == totals and sess.counters() == counters
    q1 = sess.read_queues()
    np.testing.assert_array_equal(q1[:, 0], q0[:, 0])
    np.testing.assert_array_equal(q1[:, 1, 6], np.maximum(upto[22, 1], upto[19, 1]))  # connect status follows the deliveries
    assert (q1[:, 1, 0] == q1[:, 1, 6]).all() and (q1[:, 1, 2] >= q0[:, 1, 2]).all() and (q1[:, 1, 2] > q0[:, 1, 2]).any()
    np.testing.assert_array_equal(sess.parked_ticks(), 3)
    sess.close()


def everything(sess, time_sync):
    out = dict(zip(("tags", "imgs", "cs", "live", "cur", "conf", "st", "lf", "na", "ns"), snapshot(sess)))
    out["queues"] = sess.read_queues()
    out["totals"] = np.array(sess.totals(), np.uint64)
    out["counters"] = np.array(sess.counters(), np.uint32)
    if time_sync:
        out.update(gpu_state(sess))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("time_sync", [False, True], ids=["plain", "time_sync"])
def test_gpu_no_mask_and_a_mask_of_ones_equal_run_ticks(gpu_available, time_sync):
    P, mask, d, rd, ticks = 2, 0b01, 1, 1, 90
    inputs, upto, rin = network(P, mask, rd, ticks=ticks)
    di, du, dr = dev(inputs, upto, rin)
    ones = dev(np.ones((1, S), np.uint8))
    twin, none, full = (make_session(G.Game.EX_GAME, P, mask, d, rd, time_sync=time_sync) for _ in range(3))
    if time_sync:
        rtt, adv = dev(np.full(S, 40, np.int32), np.where(np.arange(S) % 2, 6, -3).astype(np.int32))
        for b in (twin, none, full):
            b.receive_quality(1, rtt, adv)
    saw_threshold = saw_load = False
    for t in range(ticks):
        twin.run_ticks(di[t:t + 1], du[t:t + 1], dr)
        none.run_ticks(di[t:t + 1], du[t:t + 1], dr, run_mask=None)
        full.advance_frame(di[t], du[t], dr, run=ones[0])
        want = everything(twin, time_sync)
        for name, b in (("no mask", none), ("all ones", full)):
            got = everything(b, time_sync)
            for k in want:
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k}, {name}, tick {t}")
        saw_threshold |= bool((want["st"] == 1).any())
        saw_load |= bool((want["lf"] >= 0).any())
    assert saw_threshold and saw_load
    assert (full.parked_ticks() == 0).all() and (none.parked_ticks() == 0).all()
    for b in (twin, none, full):
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("time_sync", [False, True], ids=["plain", "time_sync"])
def test_gpu_one_paced_call_of_7_ticks_equals_7_one_tick_calls(gpu_available, time_sync):
    P, mask, d, rd, ticks = 3, 0b001, 1, 0, 84
    inputs, upto, rin = network(P, mask, rd, ticks=ticks)
    run = schedule(ticks)
    di, du, dr = dev(inputs, upto, rin)
    masks = dev(np.stack([session_mask(r, S) for r in run]))
    one, seven = (make_session(G.Game.EX_GAME, P, mask, d, rd, time_sync=time_sync) for _ in range(2))
    if time_sync:
        rtt, adv = dev(np.full(S, 40, np.int32), np.where(np.arange(S) % 2, 6, -3).astype(np.int32))
        for b in (one, seven):
            for h in (1, 2):
                b.receive_quality(h, rtt, adv)
    for t0 in range(0, ticks, 7):
        for t in range(t0, t0 + 7):
            one.run_ticks(di[t:t + 1], du[t:t + 1], dr, run_mask=masks[t:t + 1])
        seven.run_ticks(di[t0:t0 + 7], du[t0:t0 + 7], dr, run_mask=masks[t0:t0 + 7])
        want, got = everything(one, time_sync), everything(seven, time_sync)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k}, ticks {t0}..{t0 + 6}")
    np.testing.assert_array_equal(one.parked_ticks(), seven.parked_ticks())
    assert (one.parked_ticks()[np.arange(S) % C != 0] > 0).all()
    if time_sync:
        assert (want["windows"] != 0).any() and (want["local_adv"] != 0).any()
    one.close()
    seven.close()


@pytest.mark.gpu
def test_gpu_a_parked_poll_that_overflows_the_queue_panics_exactly_those_sessions(gpu_available):
    """Class 3 parked for 135 ticks from tick 10 on, a delivery every tick: input_queue.rs:181 fires
    in the poll of the parked tick on which the oracle's deliver panics."""
    P, mask, d, rd, ticks = 2, 0b01, 0, 0, 160
    inputs, _, rin = synth_network(S, P, ticks, mask, rd, 1, 1)
    upto = np.full((ticks, P, S), -1, np.int32)
    upto[:, 1, :] = np.arange(ticks)[:, None] - 1  # every session receives frame t - 1 before tick t
    run = np.ones((ticks, C), bool)
    run[10:145, 3] = False
    sess = make_session(G.Game.EX_GAME, P, mask, d, rd, time_sync=False)
    cls = Classes(G.Game.EX_GAME, P, d, rd, mask, S)
    di, du, dr = dev(inputs, upto, rin)
    masks = dev(np.stack([session_mask(r, S) for r in run]))
    victims = np.arange(S) % C == 3
    panic_tick = None
    frozen = None
    for t in range(ticks):
        sess.run_ticks(di[t:t + 1], du[t:t + 1], dr, run_mask=masks[t:t + 1])
        cls.tick(t, run[t], inputs, upto, rin)
        compare_status(sess, cls, f"tick {t}")
        assert sess.counters()[2] == cls.poll_panics
        if cls.dead.any() and panic_tick is None:
            panic_tick = t
            frozen = snapshot(sess)
        if t % 16 == 15 or t == ticks - 1:
            compare_all(sess, cls, f"tick {t}")
    assert panic_tick is not None and 10 < panic_tick < 145, "the panic must come from a parked poll"
    np.testing.assert_array_equal(cls.dead, victims)
    assert cls.poll_panics == victims.sum() == sess.counters()[2]
    for o, k in zip(cls.orcs, cls.cols):  # every session of the class did panic in the oracle
        assert ((o.advance()[0] == O.KIND_PANIC) == victims[k]).all()
    st = sess.status()[0]
    assert (st[victims] == L.RB_PANIC).all() and (st[~victims] == 0).all()
    assert_frozen(frozen, snapshot(sess), victims, "the panicked sessions stay stopped")
    sess.close()
    cls.close()


@pytest.mark.gpu
def test_gpu_disconnect_player_on_a_parked_session_between_paced_ticks(gpu_available):
    P, mask, d, rd = 3, 0b001, 1, 1
    inputs, upto, rin = network(P, mask, rd)
    run = schedule()
    assert not run[22, 3] and not run[21, 3] and run[22, 0]
    sess = make_session(G.Game.EX_GAME, P, mask, d, rd, time_sync=False)
    cls = Classes(G.Game.EX_GAME, P, d, rd, mask, S)
    di, du, dr = dev(inputs, upto, rin)
    masks = dev(np.stack([session_mask(r, S) for r in run]))
    who = np.arange(S) % 8 < 4  # half of every class, the parked class 3 included
    for t in range(T):
        if t == 22:
            sess.disconnect_player(2, who)
            cls.disconnect(2, who)
        sess.run_ticks(di[t:t + 1], du[t:t + 1], dr, run_mask=masks[t:t + 1])
        cls.tick(t, run[t], inputs, upto, rin)
        compare_all(sess, cls, f"tick {t}")
    # (a disconnect whose frame is the parked session's current frame trips load_frame's assert in the
    # reference, sync_layer.rs:141-145, at the session's next advance_frame: device and oracle agree above)
    parked = who & (np.arange(S) % C == 3)
    assert (sess.read_queues()[who, 2, 7] == 1).all() and not cls.dead[~who].any() and (~cls.dead[parked]).any()
    sess.close()
    cls.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["exgame_p2", "exgame_p3_disconnect", "exgame_p3_peer_status"])
def test_gpu_time_sync_under_paced_ticks_against_the_model(gpu_available, case):
    """Every tick's frames_ahead, advantages, sums (through the windows), windows and events.  A
    parked tick applies update_local_frame_advantage only.  The peer-status case has sessions that
    panic after the threshold decision inside a paced tick (the early-frame report of
    tests/test_time_sync.py): the time-sync launch must see that panic, which only the status view
    holds until the view is copied back."""
    import torch
    c = {"exgame_p2": dict(P=2, mask=0b01, D=0, RD=1),
         "exgame_p3_disconnect": dict(P=3, mask=0b001, D=1, RD=0, disconnect=(50, 1)),
         "exgame_p3_peer_status": dict(peer=True, desync=10, **PEER)}[case]
    P, mask, D, RD, ticks = c["P"], c["mask"], c["D"], c["RD"], 150
    remotes = [h for h in range(P) if not (mask >> h) & 1]
    inputs, upto, rin = network(P, mask, RD, ticks=ticks)
    run = schedule(ticks)
    sess = make_session(G.Game.EX_GAME, P, mask, D, RD, peer=c.get("peer", False), desync=c.get("desync", 0))
    model = BatchModel(S, P, mask, D, 60)
    di, du, dr = dev(inputs, upto, rin)
    masks = dev(np.stack([session_mask(r, S) for r in run]))
    cls_of = np.arange(S) % C
    panicked_at = np.full(S, -1)
    half = np.arange(S) % 2 == 0
    for t in range(ticks):
        if t % 12 == 0:
            rtt = np.where(cls_of == 1, 0, 40 + 8 * (t // 12 % 3)).astype(np.int32)
            adv = np.where(np.arange(S) % 2 == 1, 12 + t // 12 % 2, -3).astype(np.int32)
            for h in remotes:
                sess.receive_quality(h, *dev(rtt, adv))
                model.receive_quality(h, rtt, adv)
        if c.get("disconnect") and t == c["disconnect"][0]:
            sess.disconnect_player(c["disconnect"][1], half)
        if c.get("peer") and t == T_REP:
            for e, last, disc in peer_reports(T_REP, upto, P, D):
                sess.receive_peer_connect_status(e, torch.from_numpy(last).cuda(), torch.from_numpy(disc).cuda())
        cur = sess.frames()[0]
        d0 = sess.read_queues()[:, :, 7]
        sess.run_ticks(di[t:t + 1], du[t:t + 1], dr, run_mask=masks[t:t + 1])
        st = sess.status()[0]
        d1 = sess.read_queues()[:, :, 7]
        ran = run[t][cls_of]
        panicked_at[(st == L.RB_PANIC) & (panicked_at < 0)] = t
        lr = last_recv_of(upto[t], rin.shape[0])
        for s, m in enumerate(model.sessions):
            if ran[s]:
                m.advance_frame(int(cur[s]), int(st[s]), d0[s], d1[s], lr[:, s])
            else:
                parked_poll(m, int(cur[s]), d0[s], lr[:, s])
        assert_same(gpu_state(sess), model.state(), f"{case}, tick {t}")
    end = gpu_state(sess)
    assert end["counts"].sum() > 0 and (end["windows"] != 0).any() and (end["frames_ahead"] > 0).any()
    if c.get("peer"):
        hit = panicked_at >= 0  # the early report panics its sessions, each inside a tick it ran
        assert hit[np.arange(S) % 4 == 2].sum() >= 8 and (panicked_at[hit] >= T_REP).all()
        assert run[panicked_at[hit], cls_of[hit]].all()
    else:
        assert (panicked_at < 0).all()
    sess.close()


@pytest.mark.gpu
def test_gpu_closed_loop_pace_feeds_the_next_mask_on_the_device(gpu_available):
    """pace() writes the next tick's mask on the device, no host copy inside the loop; the masks (read
    back once at the end), parked_ticks() and every state equal the CPU run of the same schedule."""
    import torch
    c = LOOP
    want_masks, cls, model, (inputs, upto, rin) = closed_loop_reference()
    n, ticks, P, mask = c["n"], c["ticks"], c["P"], c["mask"]
    sess = make_session(G.Game.EX_GAME, P, mask, c["D"], c["RD"], sessions=n, fps=c["fps"])
    di, du, dr = dev(inputs, upto, rin)
    sess.receive_quality(1, *dev(*loop_quality(n)))
    run = torch.ones(n, dtype=torch.uint8, device="cuda")
    log = torch.zeros((ticks, n), dtype=torch.uint8, device="cuda")
    for t in range(ticks):
        log[t].copy_(run)
        sess.advance_frame(di[t], du[t], dr, run=run)
        sess.pace(out=run)
    masks = log.cpu().numpy()
    np.testing.assert_array_equal(masks, want_masks)
    np.testing.assert_array_equal(sess.parked_ticks(), (want_masks == 0).sum(0))
    compare_all(sess, cls, "closed loop, end")
    assert_same(gpu_state(sess), model.state(), "closed loop, end")
    sess.close()


@pytest.mark.gpu
def test_gpu_validation(gpu_available):
    import torch
    P, mask = 2, 0b01
    inputs, upto, rin = network(P, mask, 0, ticks=4, stall=False)
    di, du, dr = dev(inputs, upto, rin)
    ones = torch.ones((1, S), dtype=torch.uint8, device="cuda")

    def refused(fn, text):
        with pytest.raises(InvalidRequest) as e:
            fn()
        assert text in str(e.value), str(e.value)

    fan = make_session(G.Game.EX_GAME, P, mask, 0, 0, fanout=True, time_sync=False)
    before = everything(fan, False)
    refused(lambda: fan.run_ticks(di[:1], du[:1], dr, run_mask=ones), "a batch with the fan-out takes rb_p2p_run_ticks")
    refused(lambda: fan.pace(), "time sync is off")
    after = everything(fan, False)
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    assert (fan.parked_ticks() == 0).all()
    fan.run_ticks(di[:1], du[:1], dr)  # the batch still ticks
    assert (fan.frames()[0] == 1).all()
    fan.close()

    sess = make_session(G.Game.EX_GAME, P, mask, 0, 0, time_sync=False)
    refused(lambda: sess.pace(), "time sync is off")
    lib = L.load()
    st = lib.rb_p2p_run_ticks_paced(sess._h, 1, None, 0, ctypes.c_void_p(du.data_ptr()), ctypes.c_void_p(dr.data_ptr()),
                                    int(dr.shape[0]), ctypes.c_void_p(ones.data_ptr()))
    assert st == L.RB_INVALID_REQUEST and b"missing input tensor" in lib.rb_p2p_last_error(sess._h)
    assert (sess.frames()[0] == 0).all() and (sess.parked_ticks() == 0).all()
    sess.run_ticks(di[:1], du[:1], dr, run_mask=ones)
    assert (sess.frames()[0] == 1).all() and (sess.status()[0] == 0).all()
    sess.close()

    on = make_session(G.Game.EX_GAME, P, mask, 0, 0)
    with pytest.raises(AssertionError):
        on.pace(out=torch.ones(S + 1, dtype=torch.uint8, device="cuda"))
    assert (on.pace().cpu().numpy() == 1).all()  # nobody is ahead before the first tick
    on.close()


def parked_reports(t_rep, upto, P, D):
    """Connect-status reports (endpoint, last_frames [P, S], disconnected [P, S]) given before tick
    t_rep, shaped like tests/test_p2p_peer_status.py's: every player at the frame we hold after that
    tick's poll (a parked session polls too); endpoint 2 reports player 1 disconnected in the
    sessions s % 8 in (2, 3) at the frame we hold, and in the sessions s % 8 in (6, 7) two frames
    before it (GGRS re-triggers that disconnect every advance_frame until load_frame's assert fires)."""
    n = upto.shape[2]
    r = np.arange(n) % 8
    out = []
    for e in (1, 2):
        last = np.full((P, n), -1, np.int32)
        disc = np.zeros((P, n), np.uint8)
        for i in range(1, P):
            last[i] = np.maximum(upto[t_rep, i], -1)
        last[0] = t_rep - 1 + D
        if e == 2:
            disc[1, (r == 2) | (r == 3) | (r == 6) | (r == 7)] = 1
            early = (r == 6) | (r == 7)
            last[1, early] = upto[t_rep, 1, early] - 2
        out.append((e, last, disc))
    return out


@pytest.mark.gpu
def test_gpu_desync_detection_and_peer_reports_under_paced_ticks(gpu_available):
    """Desync detection (interval 10) and peers' connect-status reports, given at tick 62 while class
    3 is parked (a report that disconnects player 1 there takes effect at the session's next
    advance_frame): checksum reports, DesyncDetected events, disconnects and every state equal the
    class oracles' on every tick.  The peer's checksum reports are the batch's own, echoed back,
    with the checksums of a few sessions flipped from tick 50 on."""
    import torch
    from test_p2p_desync import dev_reports_as_oracle
    P, mask, D, RD = (PEER[k] for k in ("P", "mask", "D", "RD"))
    K, E, t_rep = L.RB_P2P_REPORTS_PER_TAKE, L.RB_P2P_EVENTS_KEPT, 62
    inputs, upto, rin = network(P, mask, RD)
    run = schedule()
    assert not run[t_rep, 3] and run[t_rep, 0]
    sess = make_session(G.Game.EX_GAME, P, mask, D, RD, desync=10, peer=True, time_sync=False)
    cls = Classes(G.Game.EX_GAME, P, D, RD, mask, S, desync=10)
    di, du, dr = dev(inputs, upto, rin)
    masks = dev(np.stack([session_mask(r, S) for r in run]))
    bad = np.arange(S) % 7 == 3
    dbad = dev(bad)
    for t in range(T):
        if t == t_rep:
            for e, last, disc in parked_reports(t_rep, upto, P, D):
                sess.receive_peer_connect_status(e, *dev(last, disc))
                for o, k in zip(cls.orcs, cls.cols):
                    o.receive_peer_connect_status(e, last[:, k], disc[:, k])
        sess.run_ticks(di[t:t + 1], du[t:t + 1], dr, run_mask=masks[t:t + 1])
        cls.tick(t, run[t], inputs, upto, rin)
        compare_all(sess, cls, f"tick {t}")
        a = ~cls.dead
        rep = sess.take_checksum_reports()
        gf, gc = dev_reports_as_oracle(rep)
        parts = [o.take_checksum_reports(K) for o in cls.orcs]
        of, oc = cls.gather([p[0] for p in parts], 1), cls.gather([p[1] for p in parts], 1)
        np.testing.assert_array_equal(gf[:, a], of[:, a], err_msg=f"report frames, tick {t}")
        has = (of >= 0) & a[None, :]
        np.testing.assert_array_equal(gc[has], oc[has], err_msg=f"report checksums, tick {t}")
        if t >= 50:
            rep[:, dbad, 0] ^= 1
            oc[:, bad, 0] ^= np.uint64(1)
        sess.receive_checksum_reports(1, rep)
        for o, k in zip(cls.orcs, cls.cols):
            o.receive_checksum_reports(1, np.ascontiguousarray(of[:, k]), np.ascontiguousarray(oc[:, k]))
        got = sess.desync_events()
        eparts = [o.desync_events(E) for o in cls.orcs]
        for i, what in enumerate(("counts", "frames", "handles", "local", "remote")):
            want = cls.gather([p[i] for p in eparts], 0)
            np.testing.assert_array_equal(got[i][a], want[a], err_msg=f"desync events {what}, tick {t}")
    n = sess.desync_events()[0]
    assert (n[bad & ~cls.dead] > 0).all() and (bad & ~cls.dead).sum() >= 4
    r = np.arange(S) % 8
    reported = (r == 2) | (r == 3) | (r == 6) | (r == 7)
    assert cls.dead[(r == 6) | (r == 7)].any() and not cls.dead[~reported].any()
    q = sess.read_queues()  # class 3 was parked when the reports came: disconnected by its next advance_frame
    assert (q[reported & ~cls.dead][:, 1, 7] == 1).all() and (q[~reported][:, 1, 7] == 0).all()
    assert (~cls.dead[r == 3]).any(), "a session disconnected by a report while parked must live on"
    sess.close()
    cls.close()


@pytest.mark.gpu
def test_gpu_paced_ticks_across_the_16_bit_delta_boundary(gpu_available):
    """Player 1 of a P = 3 batch is disconnected at tick 10; fused run_ticks to tick 32,700, then 200
    paced ticks, across the frame at which its frozen frames leave the 16-bit deltas of the packed
    rows (the escape rows), against the oracle on every paced tick."""
    P, mask, d, rd, n, t_paced, ticks = 3, 0b001, 1, 1, 12, 32700, 32900
    inputs, upto, rin = synth_network(n, P, ticks, mask, rd, 1, 4)
    upto[10:, 1] = upto[9, 1]  # (a disconnected player's deliveries are ignored, p2p_session.rs:852)
    run = np.ones((ticks, 2), bool)  # two classes here: never parked, and the random 30%
    run[t_paced:] = schedule(ticks - t_paced)[:, [0, 2]]
    sess = make_session(G.Game.EX_GAME, P, mask, d, rd, sessions=n, time_sync=False)
    cls = Classes(G.Game.EX_GAME, P, d, rd, mask, n, classes=2)
    di, du, dr = dev(inputs, upto, rin)
    masks = dev(np.stack([session_mask(r, n) for r in run[t_paced:]]))
    everyone = np.ones(n, bool)
    for t0 in [0, 10] + list(range(50, t_paced, 50)):
        t1 = 10 if t0 == 0 else min(t_paced, 50 if t0 == 10 else t0 + 50)
        if t0 == 10:
            sess.disconnect_player(1)
            cls.disconnect(1, everyone)
        sess.run_ticks(di[t0:t1], du[t0:t1], dr)
        for t in range(t0, t1):
            cls.tick(t, run[t], inputs, upto, rin)
    compare_all(sess, cls, f"tick {t_paced - 1}")
    escaped_before = sess.frames()[0] - sess.read_queues()[:, 1, 0] > 32767
    for t in range(t_paced, ticks):
        sess.run_ticks(di[t:t + 1], du[t:t + 1], dr, run_mask=masks[t - t_paced:t - t_paced + 1])
        cls.tick(t, run[t], inputs, upto, rin)
        compare_all(sess, cls, f"tick {t}")
    assert not escaped_before.any() and (sess.frames()[0] - sess.read_queues()[:, 1, 0] > 32767).all()
    assert not cls.dead.any() and sess.counters()[2] == 0
    assert (sess.parked_ticks()[np.arange(n) % 2 == 1] > 40).all()
    sess.close()
    cls.close()


@pytest.mark.gpu
def test_gpu_a_paced_host_feeds_spectators(gpu_available):
    """A host driven by paced ticks exports its confirmed inputs after every tick; a spectator batch
    fed from it holds, after frame c, the state of the truth's (and, once confirmed, the host's
    own) cell of frame c + 1.  A parked tick's local inputs are ignored, so the host's local input
    of frame f is the one offered on the tick that advanced frame f."""
    from test_spectator import DELAY, Feed, W_, assert_state_is_truth, host_network, host_truth, start_host, start_spectators
    game, P, mask, ticks = G.Game.EX_GAME, 2, 0b01, 90
    by_frame, upto, rin = host_network(game, P, mask, S, ticks + 8)
    run = schedule(ticks)
    ran = run[:, np.arange(S) % C]
    frame_at = np.cumsum(ran, 0) - ran  # frames advanced before tick t (lags 1-5 inside W = 8: no PredictionThreshold)
    offered = np.take_along_axis(by_frame, np.repeat(frame_at[:, None, :], P, 1), axis=0)
    host, spec = start_host(game, P, mask, S), start_spectators(game, P, S)
    di, du, dr = dev(offered, upto[:ticks], rin)
    masks = dev(ran.astype(np.uint8))
    feed = Feed(host, ticks + DELAY + 4)
    seen = host_truth(game, P, mask, by_frame, rin, ticks + 8)
    compared_host = 0
    for t in range(ticks):
        host.run_ticks(di[t:t + 1], du[t:t + 1], dr, run_mask=masks[t:t + 1])
        host.export_confirmed_inputs(feed.inputs, feed.upto, feed.last, feed.disc)
        spec.receive_host_status(feed.last.clone(), feed.disc.clone())
        spec.run_ticks(feed.upto.clone()[None], feed.inputs)
        if t % 10 == 9 or t == ticks - 1:
            assert (host.status()[0] == 0).all()
            assert_state_is_truth(spec, seen, f"tick {t}")
            cur, _ = spec.frames()
            img, cs = spec.read_live()
            tags, himg, hcs = host.read_cells()
            conf = host.frames()[1]
            for s in range(S):
                f = int(cur[s]) + 1
                if tags[f % W_, s] == f and f <= conf[s]:
                    assert np.array_equal(img[s], himg[f % W_, s]) and np.array_equal(cs[s], hcs[f % W_, s]), f"tick {t} session {s}"
                    compared_host += 1
    np.testing.assert_array_equal(host.frames()[0], ran.sum(0))
    assert spec.frames()[0].min() > 40 and compared_host > 0
    assert (host.export_status()[0] == L.RB_P2P_EXPORT_OK).all()
    host.close()
    spec.close()
