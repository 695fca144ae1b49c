"""Per-session delivery rings for P2P and spectator batches (include/ggrs_amd.h
rb_p2p_set_delivery_ring, rb_spectator_set_delivery_ring, rb_p2p_export_local_inputs; DESIGN.md
section 16).

A batch in ring mode reads its by-frame tensors as [R, P, S] rings indexed by each session's own
frame (frame f in slot f & (R - 1)), so sessions of one batch may sit any number of frames apart.
Every ring-fed batch here is compared, after every call, with the oracle and with a twin batch fed
the linear tensors; every comparison is equality.

The feeder (``Feeder``) writes each call's newly delivered frames into their slots and then
overwrites the slots of the 8 frames past the call's largest watermark with the complement of what
they held.  Those slots alias frames delivered 120 or more frames ago, and hold what a caller that
prefetches past the watermark would have put there: a consumed frame is never read again, a frame
past the watermark is loaded and discarded.  One ring tensor serves a whole run; the columns of a
restarted session keep the previous match's inputs.

R = 128 (the smallest ring), W = 8, S = 70 (two waves, one partial), 300 ticks: the ring wraps
twice.  The cohort schedule is test_restart.py's with restarts after 140 ticks (cohorts 1 and 2)
and 270 ticks (cohort 2): from tick 270 on, cohorts 0 and 2 are more than R frames apart.
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
from test_p2p import ORC_GAME, drive_oracle
from test_p2p_long_match import PLAN_TICKS
from test_p2p_pacing import compare_all, dev, everything, session_mask
from test_restart import NC, Cohorts, assembled, cohort_mask, cohort_of, match_network, phase_of
from test_time_sync import BatchModel, SessionModel, assert_same, gpu_state, make_session, quality

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, W, S, T = 128, 8, 70, 300
PAST = 8                                 # slots past a call's largest watermark the feeder spoils
RESTARTS = {140: (1, 2), 270: (2,)}      # before tick t (after t ticks): the cohorts restarted
FPS, EPOCH = 60, 12


# ---------------------------------------------------------------------------
# the feeder and the schedules
# ---------------------------------------------------------------------------
class Feeder:
    """The caller's ring [R, P, n] on the host, uploaded into ONE device tensor before every call."""

    def __init__(self, P, mask, n, dtype=np.uint8, past=PAST):
        self.ring = np.zeros((R, P, n), dtype)
        self.prev = np.full((P, n), -1, np.int64)   # newest frame delivered per endpoint
        self.remotes = [h for h in range(P) if not (mask >> h) & 1]
        self.past = past
        self.cols = np.arange(n)
        self.dev = None

    def restart(self, who):
        """The sessions `who` begin a new match.  Their columns are left as they are."""
        self.prev[:, who] = -1

    def feed(self, upto_rows, rin):
        """The deliveries of a call whose watermarks are upto_rows [k, P, n], from the linear
        by-frame tensor rin [F, P, n] of each session's current match.  Returns, per remote handle,
        (handle, first new frame [n], new frames [n])."""
        top = upto_rows.max(axis=0).astype(np.int64)
        out = []
        for h in self.remotes:
            new = np.maximum(self.prev[h], top[h])
            first, cnt = self.prev[h] + 1, new - self.prev[h]
            for k in range(int(cnt.max())):
                sel = k < cnt
                f = first[sel] + k
                self.ring[f & (R - 1), h, self.cols[sel]] = rin[f, h, self.cols[sel]]
            for k in range(1, self.past + 1):
                slot = (new + k) & (R - 1)
                self.ring[slot, h, self.cols] = ~self.ring[slot, h, self.cols]
            self.prev[h] = new
            out.append((h, first, cnt))
        return out

    def device(self):
        import torch
        if self.dev is None:
            self.dev = torch.from_numpy(self.ring.copy()).cuda()
        else:
            self.dev.copy_(torch.from_numpy(self.ring))
        return self.dev

    def move_columns(self, src, sel, dst):
        self.ring[:, :, dst] = src.ring[:, :, sel]
        self.prev[:, dst] = src.prev[:, sel]


def match_start(c, t):
    return max([0] + [r for r, who in RESTARTS.items() if c in who and r <= t])


def ring_phase(t):
    return max(p for p in [0] + sorted(RESTARTS) if p <= t)


@functools.lru_cache(maxsize=None)
def ring_assembled(P, mask, rd, n=S, dtype=np.uint8, imask=0x0F):
    """test_restart.assembled with this file's restarts and T ticks: (local inputs [T, P, n],
    remote_upto [T, P, n], {phase start: the linear remote inputs by frame of that phase})."""
    co = cohort_of(n)
    starts = [0] + sorted(RESTARTS)
    nets = {(c, m): match_network(P, mask, rd, n, c, m, T, dtype, imask)
            for c in range(NC) for m in sorted({match_start(c, t) for t in starts})}
    inputs = np.zeros((T, P, n), dtype)
    upto = np.zeros((T, P, n), np.int32)
    for t in range(T):
        for c in range(NC):
            m = match_start(c, t)
            inputs[t][:, co == c] = nets[c, m][0][t - m][:, co == c]
            upto[t][:, co == c] = nets[c, m][1][t - m][:, co == c]
    phases = {}
    for p0 in starts:
        rin = np.zeros((T + rd, P, n), dtype)
        for c in range(NC):
            rin[:, :, co == c] = nets[c, match_start(c, p0)][2][:, :, co == c]
        phases[p0] = rin
    for a in (inputs, upto, *phases.values()):
        a.setflags(write=False)
    return inputs, upto, phases


def split_calls(k, ticks=T, cuts=()):
    """Calls of k ticks over [0, ticks) that begin anew at every cut."""
    edges = [0] + sorted(c for c in cuts if 0 < c < ticks) + [ticks]
    return [(a, min(a + k, e1)) for e0, e1 in zip(edges, edges[1:]) for a in range(e0, e1, k)]


class Groups(Cohorts):
    """test_restart.Cohorts with `groups` oracles (a multiple of 3): session s is in group
    s % groups, whose cohort is group % 3.  33 groups park one session in 11 at a time."""

    def __init__(self, game, P, d, rd, mask, n, sparse=False, desync=0, groups=NC):
        super().__init__(game, P, d, rd, mask, n, sparse=sparse)
        for o in self.orcs:
            o.close()
        make = self._make

        def made(k):
            o = make(k)
            if desync:
                o.set_desync_detection(desync)
            return o

        self._make = made
        self.cols = [np.arange(c, n, groups) for c in range(groups)]
        self.orcs = [made(len(k)) for k in self.cols]

    def restart(self, cohorts):
        for g, k in enumerate(self.cols):
            if g % NC in cohorts:
                self.orcs[g].close()
                self.orcs[g] = self._make(len(k))
                self.st[k] = 0
                self.lf[k] = self.na[k] = self.ns[k] = -1
                self.dead[k] = False
        self._rin = (None, {})


def equal_everything(ring, twin, time_sync, what):
    want, got = everything(twin, time_sync), everything(ring, time_sync)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k}: ring-fed against linear-fed, {what}")
    return want


def run_calls(ring, twin, cls, feeder, inputs, upto, rin_of, calls, restarts=None, run=None, model=None, what=""):
    """The calls [(t0, t1)] on the ring-fed batch, its linear-fed twin and the oracles; after every
    call compare_all against the oracles and every read-back against the twin.  restarts:
    {tick: cohorts} before calls that begin there; run [T, groups] bool: paced ticks; model: a
    test_time_sync.BatchModel (time sync on).  Returns (saw a rollback, saw a PredictionThreshold)."""
    n = inputs.shape[2]
    restarts = restarts or {}
    assert set(restarts) <= {c[0] for c in calls}
    di, du = dev(inputs, upto)
    linear = {}
    masks = None if run is None else dev(np.stack([session_mask(r, n) for r in run]))
    all_run = np.ones(len(cls.cols), bool)
    epoch = None
    saw_load = saw_threshold = False
    for t0, t1 in calls:
        if t0 in restarts:
            m = cohort_mask(n, restarts[t0])
            for b in (ring, twin):
                b.restart_sessions(m)
            cls.restart(restarts[t0])
            feeder.restart(m != 0)
            if model is not None:
                for s in np.nonzero(m)[0]:
                    model.sessions[s] = SessionModel(model.P, model.mask, ring.input_delay, FPS)
                epoch = None
            compare_all(ring, cls, f"{what}, restart before tick {t0}")
        if model is not None and t0 // EPOCH != epoch:
            epoch = t0 // EPOCH
            for h in feeder.remotes:
                rtt, adv = quality(epoch, h, n)
                for b in (ring, twin):
                    b.receive_quality(h, *dev(rtt, adv))
                model.receive_quality(h, rtt, adv)
        rin = rin_of(t0)
        feeder.feed(upto[t0:t1], rin)
        if id(rin) not in linear:
            linear[id(rin)] = dev(rin)
        rm = None if masks is None else masks[t0:t1]
        ring.run_ticks(di[t0:t1], du[t0:t1], feeder.device(), run_mask=rm)
        twin.run_ticks(di[t0:t1], du[t0:t1], linear[id(rin)], run_mask=rm)
        for t in range(t0, t1):
            cur = cls.frames()[0] if model is not None else None
            cls.tick(t, all_run if run is None else run[t], inputs, upto, rin)
            saw_load |= bool((cls.lf >= 0).any())
            saw_threshold |= bool((cls.st == 1).any())
            if model is not None:
                nobody = np.zeros((n, model.P), bool)
                model.tick(cur, cls.st, nobody, nobody, upto[t])
        compare_all(ring, cls, f"{what}, ticks {t0}..{t1 - 1}")
        equal_everything(ring, twin, model is not None, f"{what}, ticks {t0}..{t1 - 1}")
        if model is not None:
            assert_same(gpu_state(ring), model.state(), f"{what}: time sync against the model, ticks {t0}..{t1 - 1}")
    return saw_load, saw_threshold


def start_pair(game, P, mask, d, rd, n=S, **kw):
    """(ring-fed batch, linear-fed twin) of one configuration."""
    kw.setdefault("time_sync", False)
    ring, twin = (make_session(game, P, mask, d, rd, sessions=n, **kw) for _ in range(2))
    ring.set_delivery_ring(R)
    return ring, twin


def net_kind(game):
    return (np.uint32, 0x3) if game == G.Game.STUB else (np.uint8, 0x0F)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_header_signatures_and_methods():
    header = open(os.path.join(ROOT, "include", "ggrs_amd.h")).read()
    assert re.search(r"rb_status rb_p2p_set_delivery_ring\(rb_p2p\* b, int32_t ring_frames\);", header)
    assert re.search(r"rb_status rb_spectator_set_delivery_ring\(rb_spectator\* b, int32_t ring_frames\);", header)
    assert re.search(r"rb_status rb_p2p_export_local_inputs\(rb_p2p\* b, void\* inputs_by_frame, int32_t frames, "
                     r"int32_t\* sent\);", header)
    lib = L.load()
    sig = {name: (res, args) for name, res, args in L.SIGNATURES}
    P_, I_ = ctypes.c_void_p, ctypes.c_int32
    for name, args in (("rb_p2p_set_delivery_ring", [P_, I_]), ("rb_spectator_set_delivery_ring", [P_, I_]),
                       ("rb_p2p_export_local_inputs", [P_, P_, I_, P_])):
        assert sig[name] == (I_, args)
        fn = getattr(lib, name)
        assert fn.restype is I_ and fn.argtypes == args
    assert hasattr(G.P2PSession, "set_delivery_ring") and hasattr(G.SpectatorSession, "set_delivery_ring")
    assert hasattr(G.P2PSession, "export_local_inputs") and hasattr(G, "DeliveryRing")
    assert L.RB_INPUT_QUEUE_LENGTH == R == 128


@pytest.mark.parametrize("k", [1, 7, 29])
def test_feeder_read_back_through_the_mask_reproduces_the_linear_tensors(k):
    """Read through f & (R - 1) right after the call that delivers them, the frames are those of the
    linear tensors, for test_restart.assembled's own schedule (130 ticks, restarts after 37 and 90)
    and for this file's; and every frame up to the final watermark was delivered exactly once."""
    import test_restart as TR
    P, mask, rd = 2, 0b01, 1
    inputs, upto, phases, _ = assembled(P, mask, rd)
    runs = [(TR.T, TR.RESTARTS, upto, lambda t: phases[phase_of(t)])]
    rinputs, rupto, rphases = ring_assembled(P, mask, rd)
    runs.append((T, RESTARTS, rupto, lambda t: rphases[ring_phase(t)]))
    for ticks, restarts, up, rin_of in runs:
        fd = Feeder(P, mask, S)
        seen = np.zeros((ticks + rd + 1, P, S), np.int32)
        for t0, t1 in split_calls(k, ticks, restarts):
            if t0 in restarts:
                who = cohort_mask(S, restarts[t0]) != 0
                fd.restart(who)
                seen[:, :, who] = 0
            rin = rin_of(t0)
            before = fd.ring.copy()
            for h, first, cnt in fd.feed(up[t0:t1], rin):
                assert cnt.max() <= R - PAST
                for s in range(S):
                    f = first[s] + np.arange(cnt[s])
                    np.testing.assert_array_equal(fd.ring[f & (R - 1), h, s], rin[f, h, s])
                    seen[f, h, s] += 1
                    spoiled = (first[s] + cnt[s] - 1 + np.arange(1, PAST + 1)) & (R - 1)
                    spoiled = spoiled[~np.isin(spoiled, f & (R - 1))]  # (a slot written and spoiled in one call)
                    np.testing.assert_array_equal(fd.ring[spoiled, h, s], ~before[spoiled, h, s])
        for h in fd.remotes:
            for s in range(S):
                assert (seen[:fd.prev[h, s] + 1, h, s] == 1).all() and (seen[fd.prev[h, s] + 1:, h, s] == 0).all()
        assert (fd.prev[fd.remotes] >= R).any(), "the ring wrapped"


def test_cohort_schedule_puts_sessions_of_one_batch_more_than_a_ring_apart():
    """On frame counts alone: after the restart at tick 270 cohort 0 is at least R frames ahead of
    cohort 2, so no linear tensor of R frames (no window of absolute frames) serves both."""
    P, mask, d, rd = 2, 0b01, 0, 1
    inputs, upto, phases = ring_assembled(P, mask, rd)
    cls = Cohorts(G.Game.EX_GAME, P, d, rd, mask, S)
    apart = 0
    for t in range(T):
        if t in RESTARTS:
            cls.restart(RESTARTS[t])
        cls.tick(t, np.ones(NC, bool), inputs, upto, phases[ring_phase(t)])
        cur = cls.frames()[0]
        newest = upto[t][1]  # the frames the call reads lie between the sessions' watermarks
        apart += int(cur.max() - cur.min() >= R and newest.max() - newest.min() >= R)
    assert not cls.dead.any() and apart >= 20
    co = cohort_of(S)
    assert cur[co == 0].min() > 2 * R and cur[co == 2].max() < 40
    cls.close()


LOOP = dict(P=2, D=0, ticks=T, restart=140)


def loop_lag(n=S):
    return 1 + np.arange(n) % 4


def loop_network(n=S):
    """The closed loop in closed form.  Both sides advance one frame per tick (no
    PredictionThreshold: the witness below), so after k ticks of a match a side has sent its frames
    0 .. k - 1, and what left `lag` ticks ago arrives now: at match tick m the other side's
    watermark is m - lag - 1.  Pairs s % 3 == 1 restart on both sides after 140 ticks.  Returns
    (X [T, 2, n]: side A's local inputs in row 0, side B's in row 1; upto [T, 2, n]; {phase start:
    linear inputs by frame [T, 2, n]})."""
    X = G.synth_inputs(n, 2, LOOP["ticks"], seed=SEED ^ 0x100F)
    co = cohort_of(n)
    start = np.zeros((LOOP["ticks"], n), np.int64)
    start[LOOP["restart"]:, co == 1] = LOOP["restart"]
    m = np.arange(LOOP["ticks"])[:, None] - start
    up = np.maximum(m - loop_lag(n)[None, :] - 1, -1).astype(np.int32)
    upto = np.stack([up, up], axis=1)
    late = X.copy()
    k = LOOP["ticks"] - LOOP["restart"]
    late[:k][:, :, co == 1] = X[LOOP["restart"]:][:, :, co == 1]
    for a in (X, upto, late):
        a.setflags(write=False)
    return X, upto, {0: X, LOOP["restart"]: late}


def loop_sides(n=S):
    return [Cohorts(G.Game.EX_GAME, 2, LOOP["D"], LOOP["D"], mask, n) for mask in (0b01, 0b10)]


def test_closed_loop_schedule_has_no_prediction_threshold_tick_on_the_oracle():
    X, upto, phases = loop_network()
    sides = loop_sides()
    co = cohort_of(S)
    for t in range(LOOP["ticks"]):
        if t == LOOP["restart"]:
            for c in sides:
                c.restart((1,))
        rin = phases[LOOP["restart"] if t >= LOOP["restart"] else 0]
        for c in sides:
            c.tick(t, np.ones(NC, bool), X, upto, rin)
            assert (c.st == 0).all(), f"tick {t}"
            want = np.where((co == 1) & (t >= LOOP["restart"]), t - LOOP["restart"], t) + 1
            np.testing.assert_array_equal(c.frames()[0], want)
            # what a side has sent after this tick is what the closed form says arrives `lag` ticks later
            h = 0 if c.mask == 0b01 else 1
            np.testing.assert_array_equal(c.queues()[:, h, 6], want - 1 + LOOP["D"])
    assert all((c.lf >= 0).any() for c in sides), "mispredictions roll back"
    for c in sides:
        c.close()


# ---------------------------------------------------------------------------
# GPU 1: validation
# ---------------------------------------------------------------------------
def refused(fn):
    with pytest.raises(G.InvalidRequest):
        fn()


def raw_run_ticks(sess, local, upto, rin, frames):
    return sess._lib.rb_p2p_run_ticks(sess._h, 1, ctypes.c_void_p(local.data_ptr()),
                                      sess.num_players * sess.num_sessions * local.element_size(),
                                      ctypes.c_void_p(upto.data_ptr()), ctypes.c_void_p(rin.data_ptr()), frames)


@pytest.mark.gpu
def test_gpu_validation_and_switching_back_to_linear(gpu_available):
    import torch
    P, mask, d, rd, ticks = 2, 0b01, 1, 1, 60
    inputs, upto, rin = synth_network(S, P, ticks, mask, rd, 1, 4)
    di, du, dr = dev(inputs, upto, rin)
    sess, twin = (make_session(G.Game.EX_GAME, P, mask, d, rd, time_sync=False) for _ in range(2))
    assert sess.delivery_ring == 0
    for bad in (64, 96, 1, -128, 129, 127, 192):
        refused(lambda: sess.set_delivery_ring(bad))
        assert sess.delivery_ring == 0
    for good in (0, 256, 128):
        sess.set_delivery_ring(good)
        assert sess.delivery_ring == good
    refused(lambda: sess.set_delivery_ring(96))  # nothing changed: still a ring of 128
    fd = Feeder(P, mask, S)
    fd.feed(upto[0:1], rin)
    assert raw_run_ticks(sess, di[0:1], du[0:1], dr, int(dr.shape[0])) == L.RB_INVALID_REQUEST  # a linear tensor by mistake
    assert raw_run_ticks(sess, di[0:1], du[0:1], fd.device(), 2 * R) == L.RB_INVALID_REQUEST
    with pytest.raises(AssertionError):
        sess.run_ticks(di[0:1], du[0:1], dr)
    feed = torch.zeros((R + 1, P, S), dtype=torch.uint8, device="cuda")
    marks = torch.zeros((P, S), dtype=torch.int32, device="cuda")
    assert sess._lib.rb_p2p_export_local_inputs(sess._h, ctypes.c_void_p(feed.data_ptr()), R + 1,
                                                ctypes.c_void_p(marks.data_ptr())) == L.RB_INVALID_REQUEST
    assert sess._lib.rb_p2p_export_confirmed_inputs(sess._h, ctypes.c_void_p(feed.data_ptr()), R + 1,
                                                    ctypes.c_void_p(marks.data_ptr()), ctypes.c_void_p(marks.data_ptr()),
                                                    ctypes.c_void_p(feed.data_ptr())) == L.RB_INVALID_REQUEST
    assert (sess.frames()[0] == 0).all(), "a refused call runs nothing"
    for t in range(ticks):
        if t == 20:
            sess.set_delivery_ring(0)   # back to linear between calls ...
        if t == 40:
            sess.set_delivery_ring(R)   # ... and to the ring again: the span since the last delivery is in its slots
        if sess.delivery_ring:
            fd.feed(upto[t:t + 1], rin)
            sess.run_ticks(di[t:t + 1], du[t:t + 1], fd.device())
        else:
            fd.feed(upto[t:t + 1], rin)
            sess.run_ticks(di[t:t + 1], du[t:t + 1], dr)
        twin.run_ticks(di[t:t + 1], du[t:t + 1], dr)
        equal_everything(sess, twin, False, f"tick {t}")
    spec = G.SessionBuilder(G.Game.EX_GAME, num_sessions=S).with_num_players(P).start_spectator_session()
    for bad in (64, 96, 129):
        refused(lambda: spec.set_delivery_ring(bad))
        assert spec.delivery_ring == 0
    for good in (256, 0, 128):
        spec.set_delivery_ring(good)
    up = torch.full((1, S), -1, dtype=torch.int32, device="cuda")
    assert spec._lib.rb_spectator_run_ticks(spec._h, 1, ctypes.c_void_p(up.data_ptr()), ctypes.c_void_p(feed.data_ptr()),
                                            R + 1) == L.RB_INVALID_REQUEST
    for b in (sess, twin, spec):
        b.close()


@pytest.mark.gpu
def test_gpu_delivery_ring_helper_scatters_what_the_feeder_writes(gpu_available):
    """ggrs_amd.DeliveryRing, on the device, against the host feeder (without its spoiling): ring
    and watermarks after every call of 7 ticks of the cohort schedule, 1- and 4-byte inputs."""
    import torch
    P, mask, rd = 2, 0b01, 1
    for dtype, imask, tdt in ((np.uint8, 0x0F, torch.uint8), (np.uint32, 0x3, torch.int32)):
        inputs, upto, phases = ring_assembled(P, mask, rd, S, dtype, imask)
        fd = Feeder(P, mask, S, dtype, past=0)
        ring = G.DeliveryRing(R, P, S, dtype=tdt)
        cols = np.arange(S)
        for t0, t1 in split_calls(7, T, RESTARTS):
            if t0 in RESTARTS:
                who = cohort_mask(S, RESTARTS[t0]) != 0
                fd.restart(who)
                ring.restart(who)
            rin = phases[ring_phase(t0)]
            for h, first, cnt in fd.feed(upto[t0:t1], rin):
                K = max(int(cnt.max()), 1)
                f = np.minimum(first[None, :] + np.arange(K)[:, None], rin.shape[0] - 1)
                vals = np.ascontiguousarray(rin[f, h, cols[None, :]])
                ring.scatter(h, *dev(first.astype(np.int32), cnt.astype(np.int32)), dev(vals.view(np.int32) if dtype == np.uint32 else vals))
            np.testing.assert_array_equal(ring.inputs.cpu().numpy().view(dtype), fd.ring, err_msg=f"ticks {t0}..{t1 - 1}")
            np.testing.assert_array_equal(ring.upto.cpu().numpy()[1], fd.prev[1], err_msg=f"ticks {t0}..{t1 - 1}")
        assert (ring.upto.cpu().numpy()[0] == -1).all()


# ---------------------------------------------------------------------------
# GPU 2: past the wrap
# ---------------------------------------------------------------------------
E, ST = G.Game.EX_GAME, G.Game.STUB
WRAP_ROWS = [  # name, game, P, mask, d, rd, make_session options, plans
    ("exgame-p2", E, 2, 0b01, 1, 1, {}, ("live", "q", "cells", "cells-lockstep")),
    ("exgame-p2-sparse", E, 2, 0b10, 2, 1, dict(sparse=True), ("live", "q", "cells")),
    ("exgame-p4-fanout-per-player", E, 4, 0b0001, 1, 1, dict(fanout="per-player"), ("live", "cells")),
    ("stub", ST, 2, 0b01, 1, 0, {}, ("live", "cells")),
    ("exgame-p3-net", E, 3, 0b001, 1, 2, dict(desync=10, peer=True), ("live", "q")),
]
WRAP_CASES = [r[:7] + (plan,) for r in WRAP_ROWS for plan in r[7]]


def start_wrap_pair(game, P, mask, d, rd, opts):
    if opts.get("fanout") != "per-player":
        return start_pair(game, P, mask, d, rd, **opts)
    out = []
    for _ in range(2):
        b = (G.SessionBuilder(game, num_sessions=S).with_num_players(P).with_max_prediction_window(W)
             .with_input_delay(d).with_remote_input_delay(rd).with_speculative_fanout(True, adaptive=False, per_player=True))
        for h in range(P):
            b.add_player(PlayerType.Local if (mask >> h) & 1 else PlayerType.Remote, h)
        out.append(b.start_p2p_session())
    out[0].set_delivery_ring(R)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", WRAP_CASES, ids=[f"{c[0]}-{c[7]}" for c in WRAP_CASES])
def test_gpu_ring_fed_long_match_equals_oracle_and_linear_twin(gpu_available, monkeypatch, case):
    name, game, P, mask, d, rd, opts, plan = case
    if plan.startswith("cells"):  # lane-asynchronous ticks unless lock-step
        monkeypatch.setenv("RB_P2P_SYNC_TICKS", "1" if plan == "cells-lockstep" else "0")
    dtype, imask = net_kind(game)
    inputs, upto, rin = synth_network(S, P, T, mask, rd, 1, 5, dtype=dtype, mask=imask)
    who = np.arange(S) % 5 == 1   # a stall longer than the window, across frame 128
    for h in range(P):
        if not (mask >> h) & 1:
            upto[120:133, h, who] = upto[119, h, who]
            break
    ring, twin = start_wrap_pair(game, P, mask, d, rd, opts)
    cls = Groups(game, P, d, rd, mask, S, sparse=opts.get("sparse", False), desync=opts.get("desync", 0))
    fd = Feeder(P, mask, S, dtype)
    saw_load, saw_threshold = run_calls(ring, twin, cls, fd, inputs, upto, lambda t: rin,
                                        split_calls(PLAN_TICKS[plan]), what=f"{name}, {plan}")
    assert saw_load and saw_threshold and not cls.dead.any() and ring.counters()[2] == 0
    assert (ring.frames()[0] > 2 * R).all(), "the ring wrapped twice"
    if opts.get("fanout"):
        assert ring.totals()[3] > 0
    for b in (ring, twin):
        b.close()
    cls.close()


# ---------------------------------------------------------------------------
# GPU 3: sessions far apart in one ring
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "time_sync", "paced"])
@pytest.mark.parametrize("k", [1, 7])
def test_gpu_cohorts_a_ring_apart_share_one_ring(gpu_available, k, mode):
    P, mask, d, rd = 2, 0b01, 1, 1
    inputs, upto, phases = ring_assembled(P, mask, rd)
    ring, twin = start_pair(G.Game.EX_GAME, P, mask, d, rd, time_sync=mode == "time_sync")
    groups = 33 if mode == "paced" else NC
    cls = Groups(G.Game.EX_GAME, P, d, rd, mask, S, groups=groups)
    run = None
    if mode == "paced":  # one session in 11 parked, in turn: group g sits out the ticks t % 11 == g % 11
        run = np.arange(T)[:, None] % 11 != np.arange(groups)[None, :] % 11
    model = BatchModel(S, P, mask, d, FPS) if mode == "time_sync" else None
    fd = Feeder(P, mask, S)
    saw_load, saw_threshold = run_calls(ring, twin, cls, fd, inputs, upto, lambda t: phases[ring_phase(t)],
                                        split_calls(k, T, RESTARTS), restarts=RESTARTS, run=run, model=model,
                                        what=f"{mode}, {k}-tick calls")
    assert saw_load and saw_threshold and not cls.dead.any() and ring.counters()[2] == 0
    cur, co = ring.frames()[0], cohort_of(S)
    assert cur[co == 0].min() - cur[co == 2].max() >= R, "cohorts 0 and 2 sit more than a ring apart"
    if mode == "paced":
        assert (ring.parked_ticks()[co == 0] >= T // 11 - 1).all()   # (a restart clears a session's count)
    if mode == "time_sync":
        st = gpu_state(ring)
        assert (st["counts"] > 0).any() and (st["windows"] != 0).any()
    for b in (ring, twin):
        b.close()
    cls.close()


# ---------------------------------------------------------------------------
# GPU 4: moved sessions
# ---------------------------------------------------------------------------
def check_cols(sess, cols, orc, ocols, last, what):
    """compare_all's comparisons for the sessions `cols` of a batch against the sessions `ocols` of
    one oracle batch whose last advance() returned `last`."""
    for x, y, name in zip(sess.status(), last, ("status", "load frame", "advances", "saves")):
        np.testing.assert_array_equal(x[cols], y[ocols], err_msg=f"{name}, {what}")
    tags, imgs, cs = sess.read_cells()
    otags, oimgs, ocs = (x[:, ocols] for x in orc.read_cells()[:3])
    np.testing.assert_array_equal(tags[:, cols], otags, err_msg=f"cell frames, {what}")
    valid = otags >= 0
    np.testing.assert_array_equal(imgs[:, cols][valid], oimgs[valid], err_msg=f"cell images, {what}")
    np.testing.assert_array_equal(cs[:, cols][valid], ocs[valid], err_msg=f"cell checksums, {what}")
    np.testing.assert_array_equal(sess.read_live()[cols], orc.read_live()[0][ocols], err_msg=f"live, {what}")
    for x, y in zip(sess.frames(), orc.frames()):
        np.testing.assert_array_equal(x[cols], y[ocols], err_msg=f"frames, {what}")
    dq, oq = sess.read_queues()[cols], orc.queues()[ocols]
    dq[:, :, 1] = np.where(dq[:, :, 0] < 0, oq[:, :, 1], dq[:, :, 1])  # before a queue's first add: NULL there, 0 here
    np.testing.assert_array_equal(dq, oq, err_msg=f"queues, {what}")


@pytest.mark.gpu
def test_gpu_sessions_moved_into_a_younger_ring_fed_batch(gpu_available):
    """Four sessions of batch A leave at tick 150 for columns of batch B, whose own sessions are
    at frame 20: the moved columns of the caller's ring go with them, 130 frames ahead of their
    new neighbours.  A, B and B's linear-fed twin (a 300-frame tensor) match the oracles to tick 300."""
    P, mask, d, rd, t_b, t_move = 2, 0b01, 1, 1, 130, 150
    sel, dst = np.array([3, 17, 40, 66]), np.array([0, 5, 33, 69])
    X = synth_network(S, P, T, mask, rd, 1, 4, seed=SEED ^ 0xA11)
    Y = synth_network(S, P, T, mask, rd, 1, 4, seed=SEED ^ 0xB22)
    a, a_twin = start_pair(G.Game.EX_GAME, P, mask, d, rd)
    b, b_twin = start_pair(G.Game.EX_GAME, P, mask, d, rd)
    orc_a, orc_b = (O.OracleP2P(O.EX_GAME, P, W, d, mask, S, remote_delay=rd) for _ in range(2))
    orc_m = O.OracleP2P(O.EX_GAME, P, W, d, mask, len(sel), remote_delay=rd)
    Xm = tuple(np.ascontiguousarray(x[:, :, sel]) for x in X)
    fa, fb = Feeder(P, mask, S), Feeder(P, mask, S)
    dxi, dxu, dxr = dev(*X)
    Zr = Y[2].copy()
    Zr[:, :, dst] = X[2][:, :, sel]
    dyr, dzr = dev(Y[2], Zr)
    everyone, rest = np.arange(S), np.setdiff1d(np.arange(S), dst)
    for t in range(T):
        if t == t_move:
            records = a.export_sessions(sel)
            for x in (b, b_twin):
                x.import_sessions(dst, records)
                assert x.import_refused() == 0
            fb.move_columns(fa, sel, dst)
        fa.feed(X[1][t:t + 1], X[2])
        a.run_ticks(dxi[t:t + 1], dxu[t:t + 1], fa.device())
        a_twin.run_ticks(dxi[t:t + 1], dxu[t:t + 1], dxr)
        last_a = drive_oracle(orc_a, mask, X[0], X[1], X[2], t + 1, t0=t)[-1]
        last_m = drive_oracle(orc_m, mask, *Xm, t + 1, t0=t)[-1]
        check_cols(a, everyone, orc_a, everyone, last_a, f"A, tick {t}")
        check_cols(a, sel, orc_m, np.arange(len(sel)), last_m, f"A's leavers, tick {t}")
        equal_everything(a, a_twin, False, f"A, tick {t}")
        if t < t_b:
            continue
        u = t - t_b   # B's own tick
        zi, zu, zr = Y[0][u].copy(), Y[1][u].copy(), Y[2]
        if t >= t_move:
            zi[:, dst], zu[:, dst], zr = X[0][t][:, sel], X[1][t][:, sel], Zr
        fb.feed(zu[None], zr)
        b.run_ticks(dev(zi[None]), dev(zu[None]), fb.device())
        b_twin.run_ticks(dev(zi[None]), dev(zu[None]), dzr if t >= t_move else dyr)
        last_b = drive_oracle(orc_b, mask, Y[0], Y[1], Y[2], u + 1, t0=u)[-1]
        if t >= t_move:
            check_cols(b, dst, orc_m, np.arange(len(sel)), last_m, f"B's arrivals, tick {t}")
            check_cols(b, rest, orc_b, rest, last_b, f"B's own, tick {t}")
        else:
            check_cols(b, everyone, orc_b, everyone, last_b, f"B before the move, tick {t}")
        equal_everything(b, b_twin, False, f"B, tick {t}")
    cur = b.frames()[0]
    assert cur[dst].min() - cur[rest].max() >= R and cur[dst].min() > 2 * R
    assert a.counters()[2] == 0 and b.counters()[2] == 0
    for x in (a, a_twin, b, b_twin, orc_a, orc_b, orc_m):
        x.close()


# ---------------------------------------------------------------------------
# GPU 5: spectators
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_ring_host_feeds_ring_spectators_past_the_wrap(gpu_available):
    """test_gpu_host_feeds_spectators_past_the_wrap with the host's export and the spectators'
    feed in one [R, P, S] ring, next to a linear twin of both: host calls of 13 ticks, spectators
    at catch-up speed 2, session s fed s % 4 frames short of the export."""
    import torch

    import test_spectator as TS
    game, P, mask, chunk = G.Game.EX_GAME, 2, 0b01, 13
    inputs, upto, rin = TS.host_network(game, P, mask, S, T + 8)
    hosts = [TS.start_host(game, P, mask, S) for _ in range(2)]
    specs = [TS.start_spectators(game, P, S, catchup=2) for _ in range(2)]
    hosts[0].set_delivery_ring(R)
    specs[0].set_delivery_ring(R)
    di, du, dr = dev(inputs, upto, rin)
    fd = Feeder(P, mask, S)
    feeds = [TS.Feed(hosts[0], R), TS.Feed(hosts[1], T + TS.DELAY + 4)]
    seen = TS.host_truth(game, P, mask, inputs, rin, T + 8)
    short = dev((np.arange(S) % 4).astype(np.int32))
    compared_host = 0
    for t0 in range(0, T, chunk):
        t1 = min(t0 + chunk, T)
        fd.feed(upto[t0:t1], rin)
        hosts[0].run_ticks(di[t0:t1], du[t0:t1], fd.device())
        hosts[1].run_ticks(di[t0:t1], du[t0:t1], dr)
        equal_everything(hosts[0], hosts[1], False, f"hosts, tick {t1 - 1}")
        for host, spec, feed in zip(hosts, specs, feeds):
            host.export_confirmed_inputs(feed.inputs, feed.upto, feed.last, feed.disc)
            spec.receive_host_status(feed.last.clone(), feed.disc.clone())
            target = torch.clamp(feed.upto - short, min=G.NULL_FRAME)
            spec.run_ticks(target[None].expand(t1 - t0, S).contiguous(), feed.inputs)
        gup, lup = feeds[0].upto.cpu().numpy(), feeds[1].upto.cpu().numpy()
        np.testing.assert_array_equal(gup, lup, err_msg=f"export watermark, tick {t1 - 1}")
        for x, y in zip(hosts[0].export_status(), hosts[1].export_status()):
            np.testing.assert_array_equal(x, y)
        gin, lin = feeds[0].inputs.cpu().numpy(), feeds[1].inputs.cpu().numpy()
        for s in range(S):  # the ring holds the newest R exported frames of every session
            f = np.arange(max(0, gup[s] - R + 1), gup[s] + 1)
            np.testing.assert_array_equal(gin[f & (R - 1), :, s], lin[f, :, s], err_msg=f"export, tick {t1 - 1} session {s}")
        TS.assert_state_is_truth(specs[0], seen, f"tick {t1 - 1}")
        for x, y in zip(specs[0].frames() + specs[0].read_live() + specs[0].status() + (np.array(specs[0].totals()),),
                        specs[1].frames() + specs[1].read_live() + specs[1].status() + (np.array(specs[1].totals()),)):
            np.testing.assert_array_equal(x, y, err_msg=f"ring-fed spectators against linear-fed, tick {t1 - 1}")
        cur, _ = specs[0].frames()
        img, cs = specs[0].read_live()
        tags, himg, hcs = hosts[0].read_cells()
        _, conf = hosts[0].frames()
        for s in range(S):  # the host's own cell of frame current + 1, once confirmed
            f = int(cur[s]) + 1
            w = f % TS.W_
            if tags[w, s] == f and f <= conf[s]:
                assert np.array_equal(img[s], himg[w, s]) and np.array_equal(cs[s], hcs[w, s]), f"tick {t1 - 1} session {s}"
                compared_host += 1
    assert (hosts[0].export_status()[0] == L.RB_P2P_EXPORT_OK).all()
    assert cur.min() > 2 * R and compared_host > S and specs[0].totals()[2] == 0
    for b in hosts + specs:
        b.close()


@pytest.mark.gpu
def test_gpu_ring_export_stops_at_the_overrun_rule_like_the_linear_twin(gpu_available):
    """test_gpu_export_overwrite_rule's schedule: the first export comes after 140 ticks.  Sessions
    whose remote player stopped at frame 50 export as usual, the others report
    RB_P2P_EXPORT_OVERRUN and export nothing, in ring mode exactly as in linear mode."""
    import test_spectator as TS
    game, P, mask, ticks = G.Game.EX_GAME, 2, 0b01, 150
    inputs, upto, rin = TS.host_network(game, P, mask, S, ticks)
    stalled = np.arange(S) % 3 == 0
    upto[:, 1, stalled] = np.minimum(upto[:, 1, stalled], 50)
    hosts = [TS.start_host(game, P, mask, S) for _ in range(2)]
    hosts[0].set_delivery_ring(R)
    di, du, dr = dev(inputs, upto, rin)
    fd = Feeder(P, mask, S)
    for t0, t1 in split_calls(35, 140):
        fd.feed(upto[t0:t1], rin)
        hosts[0].run_ticks(di[t0:t1], du[t0:t1], fd.device())
        hosts[1].run_ticks(di[t0:t1], du[t0:t1], dr)
    feeds = [TS.Feed(hosts[0], R), TS.Feed(hosts[1], ticks + 8)]
    for step in range(2):
        (gin, gup, glast, gdisc), (lin, lup, llast, ldisc) = feeds[0].export(), feeds[1].export()
        for x, y in zip((gup, glast, gdisc) + hosts[0].export_status(), (lup, llast, ldisc) + hosts[1].export_status()):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(hosts[0].export_status()[0], np.where(stalled, L.RB_P2P_EXPORT_OK, L.RB_P2P_EXPORT_OVERRUN))
        assert (gin[:, :, ~stalled] == feeds[0].sentinel).all(), "an overrun session exports nothing"
        assert (gup[stalled] == 50).all()
        np.testing.assert_array_equal(gin[:51][:, :, stalled], lin[:51][:, :, stalled])
        assert (gin[51:][:, :, stalled] == feeds[0].sentinel).all()
        if step == 0:
            fd.feed(upto[140:], rin)
            hosts[0].run_ticks(di[140:], du[140:], fd.device())
            hosts[1].run_ticks(di[140:], du[140:], dr)
    equal_everything(hosts[0], hosts[1], False, "after 150 ticks")
    for b in hosts:
        b.close()


# ---------------------------------------------------------------------------
# GPU 6: the local-input export
# ---------------------------------------------------------------------------
EXPORT_CASES = [  # name, P, local mask, input delay, ring
    ("linear-d0", 2, 0b01, 0, False), ("linear-d2", 2, 0b10, 2, False),
    ("ring-d0", 2, 0b01, 0, True), ("ring-d2", 2, 0b10, 2, True),
    ("ring-two-locals-d1", 4, 0b0101, 1, True), ("linear-two-locals-d1", 4, 0b0101, 1, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", EXPORT_CASES, ids=[c[0] for c in EXPORT_CASES])
def test_gpu_export_local_inputs_against_the_oracles_queues(gpu_available, case):
    """After every call (one tick, and 7 ticks from tick 70 on) the rows of the local handles hold,
    at every frame up to the oracle's local_connect_status last_frame, the input the test fed for
    that frame (blank below the input delay), `sent` is that last frame, and the rows of the
    remote handles keep their sentinel in both tensors."""
    import torch
    name, P, mask, d, ring = case
    rd, ticks = 1, 160
    inputs, upto, rin = synth_network(S, P, ticks, mask, rd, 1, 4, seed=SEED ^ 0x10CA1)
    who = np.arange(S) % 5 == 1
    remote0 = [h for h in range(P) if not (mask >> h) & 1][0]
    upto[30:45, remote0, who] = upto[29, remote0, who]   # a stall: PredictionThreshold ticks add no local input
    sess = make_session(G.Game.EX_GAME, P, mask, d, rd, time_sync=False)
    orc = O.OracleP2P(O.EX_GAME, P, W, d, mask, S, remote_delay=rd)
    F = R if ring else ticks + d + 4
    fd = Feeder(P, mask, S)
    if ring:
        sess.set_delivery_ring(R)
    di, du, dr = dev(inputs, upto, rin)
    SENT = 0xA5
    out = torch.full((F, P, S), SENT, dtype=torch.uint8, device="cuda")
    sent = torch.full((P, S), -7, dtype=torch.int32, device="cuda")
    locals_ = [h for h in range(P) if (mask >> h) & 1]
    remotes = [h for h in range(P) if not (mask >> h) & 1]
    sent[locals_] = G.NULL_FRAME
    want = np.zeros((ticks + d + 4, P, S), np.uint8)   # the input of every frame of a local handle (blank below the delay)
    cols = np.arange(S)
    calls = split_calls(1, 70) + [(a, min(a + 7, ticks)) for a in range(70, ticks, 7)]
    saw_threshold = False
    for t0, t1 in calls:
        fd.feed(upto[t0:t1], rin)
        sess.run_ticks(di[t0:t1], du[t0:t1], fd.device() if ring else dr)
        for t in range(t0, t1):
            before = orc.queues()[:, :, 6].copy()
            st = drive_oracle(orc, mask, inputs, upto, rin, t + 1, t0=t)[-1][0]
            saw_threshold |= bool((st == 1).any())
            after = orc.queues()[:, :, 6]
            for h in locals_:
                added = after[:, h] > before[:, h]
                assert (after[added, h] == np.maximum(before[added, h] + 1, d)).all()
                want[after[added, h], h, cols[added]] = inputs[t, h, cols[added]]
        sess.export_local_inputs(out, sent)
        got, gs = out.cpu().numpy(), sent.cpu().numpy()
        last = orc.queues()[:, :, 6]
        for h in remotes:
            assert (got[:, h] == SENT).all() and (gs[h] == -7).all(), f"remote rows, tick {t1 - 1}"
        for h in locals_:
            np.testing.assert_array_equal(gs[h], last[:, h], err_msg=f"sent, tick {t1 - 1}")
            f = last[None, :, h] - np.arange(R if ring else F)[:, None]   # [k, S]: the frames the tensor holds
            ok = f >= 0
            slot = f & (R - 1) if ring else f
            np.testing.assert_array_equal(got[np.where(ok, slot, 0), h, cols[None, :]][ok], want[np.where(ok, f, 0), h, cols[None, :]][ok],
                                          err_msg=f"handle {h}, tick {t1 - 1}")
            if not ring:
                past = np.arange(F)[:, None] > last[None, :, h]
                assert (got[:, h][past] == SENT).all(), "nothing is written past last_frame"
    assert saw_threshold and (last[:, locals_[0]] > R).all()
    sess.close()
    orc.close()


@pytest.mark.gpu
def test_gpu_export_local_inputs_skips_frames_the_input_queue_no_longer_holds(gpu_available):
    """A first export after 150 ticks: only last_frame - 127 .. last_frame are written (the older
    slots of the 128-entry InputQueue were overwritten), `sent` says last_frame; a caller that
    restarts a session and its `sent` entry gets the new match from frame 0."""
    import torch
    P, mask, d, rd, ticks = 2, 0b01, 0, 1, 150
    inputs, upto, rin = synth_network(S, P, ticks + 10, mask, rd, 1, 3, seed=SEED ^ 0x5C1)
    sess = make_session(G.Game.EX_GAME, P, mask, d, rd, time_sync=False)
    di, du, dr = dev(inputs, upto, rin)
    sess.run_ticks(di[:ticks], du[:ticks], dr)
    out = torch.full((ticks + 10, P, S), 0xA5, dtype=torch.uint8, device="cuda")
    sent = torch.full((P, S), G.NULL_FRAME, dtype=torch.int32, device="cuda")
    sess.export_local_inputs(out, sent)
    got, last = out.cpu().numpy(), sess.read_queues()[:, 0, 6]
    np.testing.assert_array_equal(sent.cpu().numpy()[0], last)
    assert (last > R).all()
    for s in range(S):   # (no PredictionThreshold at lags 1-3: frame f carries tick f's input)
        assert last[s] == ticks - 1
        np.testing.assert_array_equal(got[last[s] - 127:last[s] + 1, 0, s], inputs[last[s] - 127:last[s] + 1, 0, s])
        assert (got[:last[s] - 127, 0, s] == 0xA5).all() and (got[last[s] + 1:, 0, s] == 0xA5).all()
    who = np.arange(S) % 3 == 1
    sess.restart_sessions(who)
    sent[:, dev(who)] = G.NULL_FRAME
    # the restarted sessions replay the match from its tick 0, the others go on with ticks 150 .. 159
    li = np.where(who[None, None, :], inputs[:10], inputs[ticks:ticks + 10])
    lu = np.where(who[None, None, :], upto[:10], upto[ticks:ticks + 10])
    sess.run_ticks(dev(li), dev(lu), dr)
    sess.export_local_inputs(out, sent)
    got = out.cpu().numpy()
    np.testing.assert_array_equal(sent.cpu().numpy()[0], np.where(who, 9, ticks + 9))
    np.testing.assert_array_equal(got[ticks:ticks + 10, 0][:, ~who], inputs[ticks:ticks + 10, 0][:, ~who])
    np.testing.assert_array_equal(got[:10, 0][:, who], inputs[:10, 0][:, who])
    sess.close()


# ---------------------------------------------------------------------------
# GPU 7: the closed loop
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_two_batches_feed_each_other_through_one_ring(gpu_available):
    """Side A (handle 0 local) and side B (handle 1 local) share one [R, 2, S] ring and one `sent`
    tensor: each exports its own row after its tick and reads the other's, and each side's
    remote_upto is the copy of `sent` from `lag` ticks ago.  Nothing else is in between: no linear
    tensor, no host-made delivery.  Each side equals an oracle fed the closed-form linear
    deliveries (valid by the CPU witness above); at the end the two sides' confirmed cells agree."""
    import torch
    X, upto, phases = loop_network()
    lag = dev(loop_lag().astype(np.int64))
    sides = []
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):  # one stream for both batches: an export is ordered against the other side's tick
        for mask in (0b01, 0b10):
            b = make_session(G.Game.EX_GAME, 2, mask, LOOP["D"], LOOP["D"], time_sync=False)
            b.set_stream(stream)
            b.set_delivery_ring(R)
            sides.append(b)
        orcs = loop_sides()
        ring = torch.full((R, 2, S), 0xEE, dtype=torch.uint8, device="cuda")
        sent = torch.full((2, S), G.NULL_FRAME, dtype=torch.int32, device="cuda")
        hist = [sent.clone() for _ in range(5)]   # hist[4 - k]: `sent` as it was k ticks ago
        dx = dev(X)
        cols = torch.arange(S, device="cuda")
        restarted = cohort_mask(S, (1,))
        for t in range(LOOP["ticks"]):
            if t == LOOP["restart"]:
                for b, c in zip(sides, orcs):
                    b.restart_sessions(restarted)
                    c.restart((1,))
                sel = dev(restarted != 0)
                for x in [sent] + hist:   # the old match's datagrams still in flight are dropped
                    x[:, sel] = G.NULL_FRAME
            rin = phases[LOOP["restart"] if t >= LOOP["restart"] else 0]
            mine = torch.stack(hist)[4 - lag, :, cols].t().contiguous()   # [2, S]: what had been sent `lag` ticks ago
            np.testing.assert_array_equal(mine.cpu().numpy(), upto[t], err_msg=f"the loop's watermarks are the closed form, tick {t}")
            for b in sides:
                b.run_ticks(dx[t:t + 1], mine[None], ring)
            for b in sides:
                b.export_local_inputs(ring, sent)
            hist = hist[1:] + [sent.clone()]
            for b, c, name in zip(sides, orcs, "AB"):
                c.tick(t, np.ones(NC, bool), X, upto, rin)
                compare_all(b, c, f"side {name}, tick {t}")
        (ta, ia, ca), (tb, ib, cb) = (b.read_cells() for b in sides)
        confirmed = np.minimum(sides[0].frames()[1], sides[1].frames()[1])
        both = (ta == tb) & (ta >= 0) & (ta <= confirmed[None, :])
        assert both.sum() > 3 * S, "the sides hold common confirmed frames"
        np.testing.assert_array_equal(ia[both], ib[both], err_msg="confirmed cells of the two sides")
        np.testing.assert_array_equal(ca[both], cb[both], err_msg="confirmed checksums of the two sides")
        assert all((c.lf >= 0).any() for c in orcs) and all(b.counters() == (0, 0, 0) for b in sides)
        cur, co = sides[0].frames()[0], cohort_of(S)
        assert (cur[co != 1] == LOOP["ticks"]).all() and (cur[co == 1] == LOOP["ticks"] - LOOP["restart"]).all()
        for b in sides + orcs:
            b.close()
