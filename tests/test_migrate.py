"""Moving running sessions between batches (include/ggrs_amd.h rb_p2p_export_sessions,
rb_p2p_import_sessions, rb_spectator_export_sessions, rb_spectator_import_sessions; DESIGN.md
section 15).  GGRS has no such call (a P2PSession is a movable Rust value), so a moved session is
defined by comparison: it continues exactly as the same session of a twin batch that was never
moved, and its new neighbours continue exactly as those of a twin that received nothing.

The batches of a move, all of the same configuration:
  A  the twin: network X in every tick
  B  the source: X; sessions `sel` are exported after T_MOVE ticks, and B goes on (export only reads)
  C  the destination: another network Y for T_MOVE ticks (its columns are dirty, at other frames),
     then the records into the sessions `dst`, then the tensors Z = X's columns sel at dst, Y elsewhere
  D  the twin of C's unselected sessions: Y in every tick
Every comparison is equality.  rb_p2p_totals and rb_p2p_counters are batch-wide and stay with
their batch; they are not compared across batches."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import ggrs_amd as G
from ggrs_amd import _lib as L
from ggrs_amd.p2p import PlayerType, synth_network
from ggrs_amd.synth import SEED
from oracle import oracle as O
from test_p2p import ORC_GAME
from test_p2p_pacing import dev, everything
from test_restart import DIRTY, PARITY, T_DISC, T_PEER, Dirty, assert_dirtied, net_kind, session_axis, start, start_dirty
from test_time_sync import make_session, peer_reports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TESTS = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(ROOT, "ggrs_amd", "csrc")
W = 8
S = 70                  # two waves, the second partial
T_MOVE, T_END = 37, 120
BATCH_WIDE = ("totals", "counters")


def selection(n):
    """Every third session, plus the first and last of each wave."""
    sel = set(range(0, n, 3))
    for w0 in range(0, n, 64):
        sel |= {w0, min(w0 + 63, n - 1)}
    return np.array(sorted(sel), np.int32)


def destinations(sel, n):
    """As many distinct sessions, in an order that sends no session to its own index: some of them
    selected themselves, some not."""
    rng = np.random.default_rng(0xD57 + n)
    while True:
        dst = rng.permutation(n)[:len(sel)].astype(np.int32)
        if (dst != sel).all() and np.isin(dst, sel).any() and not np.isin(dst, sel).all():
            return dst


@functools.lru_cache(maxsize=None)
def network(tag, P, mask, rd, n=S, ticks=T_END, dtype=np.uint8, imask=0x0F, stalls=((12, 23), (60, 75))):
    """Network `tag` (a seed): lags 1-4, the first remote handle of the sessions s % 5 == 1 stalled
    over `stalls`, each longer than the prediction window."""
    inputs, upto, rin = synth_network(n, P, ticks, mask, rd, 1, 4, seed=SEED ^ (0x3160 + 0x101 * tag), dtype=dtype, mask=imask)
    h = [x for x in range(P) if not (mask >> x) & 1][0]
    who = np.arange(n) % 5 == 1
    for t0, t1 in stalls:
        if t1 <= ticks:
            upto[t0:t1, h, who] = upto[t0 - 1, h, who]
    for a in (inputs, upto, rin):
        a.setflags(write=False)
    return inputs, upto, rin


def moved_tensors(X, Y, sel, dst):
    """Z: the caller's tensors move with the sessions: X's columns sel at dst, Y elsewhere."""
    out = []
    for x, y in zip(X, Y):
        z = y.copy()
        z[..., dst] = x[..., sel]
        out.append(z)
    return tuple(out)


def assert_columns(got, gcols, want, wcols, what):
    """Every read-back of `got` on the sessions gcols == `want`'s on wcols (index lists)."""
    assert got.keys() == want.keys()
    for k in want:
        if k in BATCH_WIDE:
            continue
        ax = session_axis(k, want[k])
        np.testing.assert_array_equal(np.take(got[k], gcols, ax), np.take(want[k], wcols, ax), err_msg=f"{k}, {what}")


def others(n, cols):
    return np.setdiff1d(np.arange(n), cols).astype(np.int32)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "ggrs_amd.h")).read()
    lib = L.load()
    sig = {name: (res, args) for name, res, args in L.SIGNATURES + L.SIZE_SIGNATURES}
    P, I = ctypes.c_void_p, ctypes.c_int32
    for kind in ("p2p", "spectator"):
        b = f"rb_{kind}"
        for decl in (rf"int64_t\s+{b}_session_record_bytes\(const {b}\* b\);",
                     rf"rb_status {b}_export_sessions\({b}\* b, const int32_t\* sessions, int32_t n, void\* records_dev\);",
                     rf"rb_status {b}_import_sessions\({b}\* b, const int32_t\* sessions, int32_t n, const void\* records_dev\);",
                     rf"rb_status {b}_import_refused\({b}\* b, uint32_t\* count\);"):
            assert re.search(decl, header), decl
        want = {f"{b}_session_record_bytes": (ctypes.c_int64, [P]), f"{b}_export_sessions": (I, [P, P, I, P]),
                f"{b}_import_sessions": (I, [P, P, I, P]), f"{b}_import_refused": (I, [P, P])}
        for name, (res, args) in want.items():
            assert sig[name] == (res, args)
            fn = getattr(lib, name)
            assert fn.restype is res and fn.argtypes == args
    for cls in (G.P2PSession, G.SpectatorSession):
        for name in ("record_bytes", "export_sessions", "import_sessions", "import_refused"):
            assert hasattr(cls, name)
    assert callable(G.move_sessions)


def test_record_layout_host_program(tmp_path):
    """tests/check_session_record.cpp over ggrs_amd/csrc/session_record.hpp: parts inside the record,
    disjoint, aligned; record_bytes a multiple of 16; the fingerprint follows every plane's shape."""
    exe = str(tmp_path / "check_session_record")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", _CSRC, "-o", exe,
                    os.path.join(_TESTS, "check_session_record.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"64 plane lists, \d+ variants, 0 failures", r.stdout)  # 4 games x 2^4 groups


def test_selection_and_destinations():
    for n in (S, 6):
        sel, dst = selection(n), destinations(selection(n), n)
        assert len(set(dst)) == len(dst) == len(sel) and (dst != sel).all()
    sel = selection(S)
    assert {0, 63, 64, 69} <= set(sel) and len(sel) == 25


# ---------------------------------------------------------------------------
# GPU 1, 10: a move continues the match
# ---------------------------------------------------------------------------
def oracle_check(sess, cols, orc, last, what):
    """compare_all (test_p2p_pacing.py) of the sessions `cols` against an oracle of len(cols) sessions."""
    for x, y, name in zip(sess.status(), last, ("status", "load frame", "advances", "saves")):
        np.testing.assert_array_equal(x[cols], y, err_msg=f"{name}, {what}")
    tags, imgs, cs = sess.read_cells()
    otags, oimgs, ocs = orc.read_cells()
    np.testing.assert_array_equal(tags[:, cols], otags, err_msg=f"cell frames, {what}")
    valid = otags >= 0
    np.testing.assert_array_equal(imgs[:, cols][valid], oimgs[valid], err_msg=f"cell images, {what}")
    np.testing.assert_array_equal(cs[:, cols][valid], ocs[valid], err_msg=f"cell checksums, {what}")
    np.testing.assert_array_equal(sess.read_live()[cols], orc.read_live()[0], err_msg=f"live, {what}")
    for x, y in zip(sess.frames(), orc.frames()):
        np.testing.assert_array_equal(x[cols], y, err_msg=f"frames, {what}")
    dq, oq = sess.read_queues()[cols], orc.queues()
    dq[:, :, 1] = np.where(dq[:, :, 0] < 0, oq[:, :, 1], dq[:, :, 1])  # before a queue's first add: NULL there, 0 here
    np.testing.assert_array_equal(dq, oq, err_msg=f"queues, {what}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(PARITY))
def test_gpu_a_moved_session_continues_its_match(gpu_available, case):
    game, P, mask, d, rd, sparse, n = PARITY[case]
    dtype, imask = net_kind(game)
    X, Y = (network(tag, P, mask, rd, n, T_END, dtype, imask) for tag in (1, 2))
    sel = selection(n)
    dst = destinations(sel, n)
    rest = others(n, dst)
    Z = moved_tensors(X, Y, sel, dst)
    a, b, c, dd = (start(game, P, mask, d, rd, sparse, n) for _ in range(4))
    dx, dy, dz = dev(*X), dev(*Y), dev(*Z)
    with_oracle = case == "exgame-p2-h0-d0"  # the chain of twins tied to the reference restatement once
    orc = O.OracleP2P(ORC_GAME[game], P, W, d, mask, len(sel), sparse_saving=sparse, remote_delay=rd) if with_oracle else None
    remotes = [h for h in range(P) if not (mask >> h) & 1]
    everyone = np.arange(n)

    def check(what):
        ea, eb, ec, ed = (everything(s, False) for s in (a, b, c, dd))
        assert_columns(ec, dst, ea, sel, f"{case}, moved, {what}")
        assert_columns(ec, rest, ed, rest, f"{case}, neighbours, {what}")
        assert_columns(eb, everyone, ea, everyone, f"{case}, source, {what}")
        return ea

    saw_load = saw_threshold = False
    for t in range(T_END):
        if t == T_MOVE:
            assert (c.read_live()[dst] != b.read_live()[sel]).any(), "the destination holds another match"
            rb = b.record_bytes
            assert rb == c.record_bytes and rb % 16 == 0
            before = everything(b, False)
            records = b.export_sessions(sel)
            assert tuple(records.shape) == (len(sel), rb) and str(records.dtype) == "torch.uint8"
            assert_columns(everything(b, False), everyone, before, everyone, f"{case}, export only reads")
            totals, counters = c.totals(), c.counters()
            c.import_sessions(dst, records)
            assert c.import_refused() == 0 and (c.totals(), c.counters()) == (totals, counters)
            check("after the import")
        for s, (di, du, dr) in ((a, dx), (b, dx), (dd, dy), (c, dz if t >= T_MOVE else dy)):
            s.run_ticks(di[t:t + 1], du[t:t + 1], dr)
        if orc is not None:
            for h in remotes:
                assert orc.deliver(h, np.ascontiguousarray(X[1][t, h][sel]), np.ascontiguousarray(X[2][:, h][:, sel])) == 0
            for h in range(P):
                if (mask >> h) & 1:
                    orc.add_local_input(h, np.ascontiguousarray(X[0][t, h][sel]))
            last = orc.advance()
            oracle_check(c if t >= T_MOVE else b, dst if t >= T_MOVE else sel, orc, last, f"{case}, oracle, tick {t}")
        if t >= T_MOVE:
            ea = check(f"tick {t}")
            saw_load |= bool((ea["lf"][sel] >= 0).any())
            saw_threshold |= bool((ea["st"][sel if n == S else everyone] == 1).any())  # (six sessions: the stalled one is not selected)
    assert saw_load and saw_threshold, "the moved sessions rolled back and stalled after the move"
    assert c.counters()[2] == 0 and (c.frames()[0][dst] > T_END - 16).all()
    for s in (a, b, c, dd):
        s.close()
    if orc is not None:
        orc.close()


# ---------------------------------------------------------------------------
# GPU 2: every feature on
# ---------------------------------------------------------------------------
DIRTY_TICKS = T_END


@functools.lru_cache(maxsize=None)
def dirty_net(match):
    """test_restart.dirty_network, long enough for T_END ticks, with a second stall after the move."""
    P, mask, rd = DIRTY["P"], DIRTY["mask"], DIRTY["RD"]
    inputs, upto, rin = synth_network(S, P, DIRTY_TICKS + 12, mask, rd, 1, 4, seed=SEED ^ (0xD1 + match))
    who = np.arange(S) % 5 == 1
    for t0, t1 in ((30, 41), (70, 81)):
        upto[t0:t1, 1, who] = upto[t0 - 1, 1, who]
    return inputs, upto, rin


class Moving(Dirty):
    """test_restart.Dirty with a feed long enough for T_END ticks, and `plays`: the session of the
    scenario (test_restart.drive_dirty's per-session events) that each column plays."""

    def __init__(self, sess, match):
        from test_spectator import Feed
        super().__init__(sess)
        self.feed = Feed(sess, DIRTY_TICKS + 32)
        self.plays = np.arange(S)
        self.nets = [tuple(a.copy() for a in dirty_net(match))]  # this batch's tensors, by column

    def tensors(self):
        return dev(*self.nets[0])

    def take(self, src, sel, dst):
        """The caller's side of a move of src's sessions sel to this batch's dst: the columns of the
        network tensors, of the run mask and of the spectators' feed, and who plays there."""
        for mine, theirs in zip(self.nets[0], src.nets[0]):
            mine[..., dst] = theirs[..., sel]
        self.plays[dst] = src.plays[sel]
        idst, isel = dev(dst.astype(np.int64)), dev(sel.astype(np.int64))
        self.run[idst] = src.run[isel]
        self.feed.inputs[:, :, idst] = src.feed.inputs[:, :, isel]
        self.feed.upto[idst] = src.feed.upto[isel]
        self.feed.last[:, idst] = src.feed.last[:, isel]
        self.feed.disc[:, idst] = src.feed.disc[:, isel]
        self.reports[:, idst] = src.reports[:, isel]


def drive_moving(batches, t0, t1):
    """test_restart.drive_dirty for batches whose columns play sessions of their own (`plays`) on
    tensors of their own: ticks [t0, t1) in lock step."""
    P, D = DIRTY["P"], DIRTY["D"]
    tens = [b.tensors() for b in batches]
    for t in range(t0, t1):
        for b, (di, du, dr) in zip(batches, tens):
            s, who = b.sess, b.plays
            if t % 12 == 0:
                rtt = dev(np.full(S, 40 + 8 * (t // 12 % 3), np.int32))
                adv = dev(np.where(who % 2 == 1, 12 + t // 12 % 2, -3).astype(np.int32))
                for h in (1, 2):
                    s.receive_quality(h, rtt, adv)
            if t == T_DISC:
                s.disconnect_player(2, who % 7 == 5)
            if t == T_PEER:
                assert (who == np.arange(S)).all(), "the peers' reports are built by column"
                for e, last, disc in peer_reports(T_PEER, b.nets[0][1], P, D):
                    s.receive_peer_connect_status(e, *dev(last, disc))
            s.advance_frame(di[t], du[t], dr, run=b.run)
            s.export_confirmed_inputs(b.feed.inputs, b.feed.upto, b.feed.last, b.feed.disc)
            b.reports = s.take_checksum_reports()
            echo = b.reports.clone()
            if t >= 20:
                echo[:, dev(who % 7 == 3), 0] ^= 1
            s.receive_checksum_reports(1, echo)
            s.pace(out=b.run)


@pytest.mark.gpu
def test_gpu_a_move_with_every_feature_on(gpu_available):
    """Desync detection, peer status, time sync, paced ticks, exports, a disconnect, panicked
    sessions and stalls.  The selection includes panicked, parked and disconnected sessions.  The
    desync events' payloads (ds_local, ds_remote) and the checksum histories behind them are what a
    forgotten carry-only plane breaks."""
    a, b, c = Moving(start_dirty(), 0), Moving(start_dirty(), 0), Moving(start_dirty(), 1)
    drive_moving([a, b, c], 0, T_MOVE)
    assert_dirtied(b)
    rb_ = b.readbacks()
    sel = selection(S)
    dst = destinations(sel, S)
    assert (rb_["st"][sel] == L.RB_PANIC).any() and (rb_["parked"][sel] > 0).any() and (rb_["queues"][sel, 2, 7] == 1).any()
    assert (rb_["ds_n"][sel] > 0).any(), "moved sessions hold desync events"
    rest = others(S, dst)
    before = c.readbacks()
    records = b.sess.export_sessions(sel)
    c.sess.import_sessions(dst, records)
    c.take(b, sel, dst)
    assert c.sess.import_refused() == 0
    assert_columns(c.readbacks(), dst, rb_, sel, "after the import")
    assert_columns(c.readbacks(), rest, before, rest, "neighbours across the import")
    # the stale mirror of ConnectionStatus::disconnected: handle 2 of the sessions that played s % 7 == 5
    # is disconnected, wherever they sit now
    was = c.plays % 7 == 5
    moved_in = np.zeros(S, bool)
    moved_in[dst] = True
    for batch, mask_ in ((c, moved_in & was), (a, np.isin(np.arange(S), sel) & (np.arange(S) % 7 == 5))):
        assert mask_.any()
        with pytest.raises(G.InvalidRequest, match="Player already disconnected."):
            batch.sess.disconnect_player(2, mask_)
    fresh_c, fresh_a = moved_in & ~was & (c.plays % 7 == 6), np.isin(np.arange(S), sel) & (np.arange(S) % 7 == 6)
    assert fresh_c.sum() == fresh_a.sum() > 0
    c.sess.disconnect_player(2, fresh_c)  # succeeds where the twin's does
    a.sess.disconnect_player(2, fresh_a)
    for t in range(T_MOVE, T_END):
        drive_moving([a, c], t, t + 1)
        assert_columns(c.readbacks(), dst, a.readbacks(), sel, f"tick {t}")
    assert (a.readbacks()["parked"][sel] > rb_["parked"][sel]).any(), "moved sessions went on parking"
    for x in (a, b, c):
        x.sess.close()


# ---------------------------------------------------------------------------
# GPU 3: launch shapes
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["exgame-p2", "exgame-p2-sparse", "brawler", "brawler-sparse"])
def test_gpu_launch_shapes_after_a_move(gpu_available, case):
    game, n = (G.Game.BRAWLER, 6) if case.startswith("brawler") else (G.Game.EX_GAME, S)
    sparse = case.endswith("sparse")
    P, mask, d, rd, ticks = 2, 0b01, 1, 1, T_MOVE + 100
    X, Y = (network(tag, P, mask, rd, n, ticks) for tag in (3, 4))
    sel = selection(n)
    dst = destinations(sel, n)
    rest = others(n, dst)
    dx, dy, dz = dev(*X), dev(*Y), dev(*moved_tensors(X, Y, sel, dst))
    for chunk in (1, 7, 50):  # kOne, kQ, LdsC|Async
        a, b, c, dd = (start(game, P, mask, d, rd, sparse, n) for _ in range(4))
        for s, (di, du, dr) in ((a, dx), (b, dx), (c, dy), (dd, dy)):
            s.run_ticks(di[:T_MOVE], du[:T_MOVE], dr)
        c.import_sessions(dst, b.export_sessions(sel))
        for t0 in range(T_MOVE, ticks, chunk):
            t1 = min(ticks, t0 + chunk)
            for s, (di, du, dr) in ((a, dx), (c, dz), (dd, dy)):
                s.run_ticks(di[t0:t1], du[t0:t1], dr)
        ea, ec, ed = (everything(s, False) for s in (a, c, dd))
        assert_columns(ec, dst, ea, sel, f"{case}, moved, launches of {chunk}")
        assert_columns(ec, rest, ed, rest, f"{case}, neighbours, launches of {chunk}")
        assert (ea["cur"][sel] > ticks - 16).all() and c.counters()[2] == 0
        for s in (a, b, c, dd):
            s.close()


# ---------------------------------------------------------------------------
# GPU 4: records are position independent
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_records_through_the_host_shuffled_into_a_batch_that_never_ticked(gpu_available):
    """The stand-in for the cross-device path of move_sessions, which one GPU cannot run: the records
    leave the device, are reordered together with their destinations and come back in a new tensor."""
    import torch
    P, mask, d, rd, ticks = 2, 0b01, 1, 1, 70
    X, Y = network(5, P, mask, rd, S, ticks), network(6, P, mask, rd, S, ticks)
    sel = selection(S)
    dst = destinations(sel, S)
    rest = others(S, dst)
    a, b = (make_session(G.Game.EX_GAME, P, mask, d, rd, time_sync=False) for _ in range(2))
    dx = dev(*X)
    for s in (a, b):
        s.run_ticks(dx[0][:T_MOVE], dx[1][:T_MOVE], dx[2])
    host_bytes = b.export_sessions(sel).cpu().numpy().copy()
    b.close()
    order = np.random.default_rng(11).permutation(len(sel))
    records = torch.from_numpy(np.ascontiguousarray(host_bytes[order])).cuda()
    e, f = (make_session(G.Game.EX_GAME, P, mask, d, rd, time_sync=False) for _ in range(2))  # created now, never ticked
    e.import_sessions(dst[order], records)
    assert e.import_refused() == 0
    assert_columns(everything(e, False), dst, everything(a, False), sel, "after the import")
    assert_columns(everything(e, False), rest, everything(f, False), rest, "fresh neighbours")
    with pytest.raises(G.InvalidRequest, match="comes before the batch's first tick"):
        e.enable_time_sync(60)  # closed as after a tick
    f.enable_time_sync(60)      # (still open on the batch that imported nothing)
    f.close()
    f = make_session(G.Game.EX_GAME, P, mask, d, rd, time_sync=False)
    # e's other sessions begin match Y at its tick 0 now
    zi, zu = Y[0][:ticks - T_MOVE].copy(), Y[1][:ticks - T_MOVE].copy()
    zr = Y[2].copy()
    zi[:, :, dst], zu[:, :, dst], zr[:, :, dst] = X[0][T_MOVE:][:, :, sel], X[1][T_MOVE:][:, :, sel], X[2][:, :, sel]
    dz, dy = dev(zi, zu, zr), dev(*Y)
    for t in range(ticks - T_MOVE):
        a.run_ticks(dx[0][T_MOVE + t:T_MOVE + t + 1], dx[1][T_MOVE + t:T_MOVE + t + 1], dx[2])
        e.run_ticks(dz[0][t:t + 1], dz[1][t:t + 1], dz[2])
        f.run_ticks(dy[0][t:t + 1], dy[1][t:t + 1], dy[2])
        ee = everything(e, False)
        assert_columns(ee, dst, everything(a, False), sel, f"moved, tick {T_MOVE + t}")
        assert_columns(ee, rest, everything(f, False), rest, f"neighbours, tick {T_MOVE + t}")
    assert e.counters()[2] == 0
    for s in (a, e, f):
        s.close()


# ---------------------------------------------------------------------------
# GPU 5: rewind
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_importing_a_batchs_own_records_rewinds_it(gpu_available):
    P, mask, d, rd, t_back = 2, 0b01, 1, 1, 60
    X = network(7, P, mask, rd, S, t_back, stalls=((12, 23), (40, 51)))
    dx = dev(*X)
    sess = make_session(G.Game.EX_GAME, P, mask, d, rd)  # time sync on
    rtt, adv = dev(np.full(S, 40, np.int32), np.where(np.arange(S) % 2, 6, -3).astype(np.int32))
    sess.receive_quality(1, rtt, adv)
    sel = selection(S)
    sess.run_ticks(dx[0][:T_MOVE], dx[1][:T_MOVE], dx[2])
    records = sess.export_sessions(sel)
    at_export = everything(sess, True)
    first = []
    for t in range(T_MOVE, t_back):
        sess.run_ticks(dx[0][t:t + 1], dx[1][t:t + 1], dx[2])
        first.append(everything(sess, True))
    assert (first[-1]["cur"][sel] > at_export["cur"][sel]).all()
    sess.import_sessions(sel, records)
    assert sess.import_refused() == 0
    assert_columns(everything(sess, True), sel, at_export, sel, "back at the export")
    assert_columns(everything(sess, True), others(S, sel), first[-1], others(S, sel), "the others stay where they were")
    for t in range(T_MOVE, t_back):
        sess.run_ticks(dx[0][t:t + 1], dx[1][t:t + 1], dx[2])
        assert_columns(everything(sess, True), sel, first[t - T_MOVE], sel, f"replayed tick {t}")
    sess.close()


# ---------------------------------------------------------------------------
# GPU 6: past the escape rows
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_a_session_behind_the_escape_bit_moves(gpu_available):
    """test_restart.py's set-up: player 1 is disconnected at tick 30; past frame 32,800 its frozen
    frames sit behind the escape bit in the absolute rows, which move with the session."""
    P, mask, d, rd, n, t_long, more = 2, 0b01, 1, 1, 12, 32800, 40
    inputs, upto, rin = synth_network(n, P, t_long + more, mask, rd, 1, 5)
    upto[30:, 1] = upto[29, 1]
    Y = synth_network(n, P, more + 20, mask, rd, 1, 4, seed=SEED ^ 0xE5D)
    sel = np.arange(1, n, 2).astype(np.int32)
    dst = np.array([0, 5, 2, 11, 7, 4], np.int32)
    rest = others(n, dst)
    b, twin, c, dd = (make_session(G.Game.EX_GAME, P, mask, d, rd, sessions=n, time_sync=False) for _ in range(4))
    di, du, dr = dev(inputs, upto, rin)
    for t0 in [0, 30] + list(range(50, t_long, 50)):
        t1 = 30 if t0 == 0 else min(t_long, 50 if t0 == 30 else t0 + 50)
        for s in (b, twin):
            if t0 == 30:
                s.disconnect_player(1)
            s.run_ticks(di[t0:t1], du[t0:t1], dr)
    assert (b.frames()[0] - b.read_queues()[:, 1, 0] > 32767).all(), "every session's player 1 escaped"
    dy = dev(*Y)
    for s in (c, dd):
        s.run_ticks(dy[0][:20], dy[1][:20], dy[2])
    G.move_sessions(b, sel, c, dst)
    # c's tensors: the moved columns play on at their own frames, the others go on with Y
    zi, zu = Y[0][20:20 + more].copy(), Y[1][20:20 + more].copy()
    zr = np.zeros_like(rin)
    zr[:Y[2].shape[0]] = Y[2]
    zi[:, :, dst], zu[:, :, dst], zr[:, :, dst] = inputs[t_long:][:, :, sel], upto[t_long:][:, :, sel], rin[:, :, sel]
    dz = dev(zi, zu, zr)
    for t in range(more):
        c.run_ticks(dz[0][t:t + 1], dz[1][t:t + 1], dz[2])
        twin.run_ticks(di[t_long + t:t_long + t + 1], du[t_long + t:t_long + t + 1], dr)
        dd.run_ticks(dy[0][20 + t:21 + t], dy[1][20 + t:21 + t], dy[2])
        ec = everything(c, False)
        assert_columns(ec, dst, everything(twin, False), sel, f"moved, tick {t}")
        assert_columns(ec, rest, everything(dd, False), rest, f"neighbours, tick {t}")
    q = c.read_queues()
    assert (q[dst, 1, 7] == 1).all() and (q[rest, 1, 7] == 0).all() and (c.frames()[0][dst] > t_long).all()
    with pytest.raises(G.InvalidRequest, match="Player already disconnected."):
        c.disconnect_player(1, np.isin(np.arange(n), dst))  # the mirror is read back from the imported rows
    assert c.counters()[2] == 0
    for s in (b, twin, c, dd):
        s.close()


# ---------------------------------------------------------------------------
# GPU 7: the fan-out
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("per_player", [True, False], ids=["per_player", "one_player"])
def test_gpu_a_move_between_fanout_batches(gpu_available, per_player):
    """The presimulated branches are not carried: an imported session has no
    valid branch, as a restarted one.  Its states equal the twin's; only rb_p2p_totals differ."""
    P, mask, d, rd = 2, 0b01, 0, 1

    def fan():
        x = (G.SessionBuilder(G.Game.EX_GAME, num_sessions=S).with_num_players(P).with_max_prediction_window(W)
             .with_input_delay(d).with_remote_input_delay(rd)
             .with_speculative_fanout(True, adaptive=False, per_player=per_player))
        for h in range(P):
            x.add_player(PlayerType.Local if (mask >> h) & 1 else PlayerType.Remote, h)
        return x.start_p2p_session()

    X, Y = network(8, P, mask, rd), network(9, P, mask, rd)
    sel = selection(S)
    dst = destinations(sel, S)
    rest = others(S, dst)
    dx, dy, dz = dev(*X), dev(*Y), dev(*moved_tensors(X, Y, sel, dst))
    a, b, c, dd = (fan() for _ in range(4))
    for t in range(T_END):
        if t == T_MOVE:
            assert b.totals()[3] > 0, "branches were selected before the move"
            c.import_sessions(dst, b.export_sessions(sel))
            assert c.import_refused() == 0
            base = c.totals()[3]
        for s, (di, du, dr) in ((a, dx), (b, dx), (dd, dy), (c, dz if t >= T_MOVE else dy)):
            s.run_ticks(di[t:t + 1], du[t:t + 1], dr)
        if t >= T_MOVE:
            ea, eb, ec, ed = (everything(s, False) for s in (a, b, c, dd))
            assert_columns(ec, dst, ea, sel, f"moved, tick {t}")
            assert_columns(ec, rest, ed, rest, f"neighbours, tick {t}")
            assert_columns(eb, np.arange(S), ea, np.arange(S), f"source, tick {t}")
    assert c.totals()[3] > base, "the destination goes on selecting branches"
    np.testing.assert_array_equal(np.array(b.totals()), np.array(a.totals()), err_msg="export leaves the source's totals alone")
    for s in (a, b, c, dd):
        s.close()


# ---------------------------------------------------------------------------
# GPU 8: spectators move with their hosts
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_spectators_move_with_their_hosts(gpu_available):
    """DESIGN.md section 11's identity for the moved pairs, after the move and through 40 more
    ticks: the spectator's state after frame c is the host's cell of frame c + 1."""
    from test_spectator import DELAY, REMOTE_DELAY, W_, Feed, start_host, start_spectators
    game, P, mask, ticks = G.Game.EX_GAME, 2, 0b01, T_MOVE + 40
    X, Y = network(10, P, mask, REMOTE_DELAY, S, ticks), network(11, P, mask, REMOTE_DELAY, S, ticks)
    sel = selection(S)
    dst = destinations(sel, S)
    idst, isel = dev(dst.astype(np.int64)), dev(sel.astype(np.int64))
    dx, dy, dz = dev(*X), dev(*Y), dev(*moved_tensors(X, Y, sel, dst))
    hb, hc = start_host(game, P, mask, S), start_host(game, P, mask, S)
    sb, sc = start_spectators(game, P, S), start_spectators(game, P, S)
    fb, fc = Feed(hb, ticks + DELAY + 4), Feed(hc, ticks + DELAY + 4)
    assert sb.record_bytes == sc.record_bytes and sb.record_bytes % 16 == 0 and sb.record_bytes != hb.record_bytes

    def tick(host, spec, feed, tensors, t):
        host.run_ticks(tensors[0][t:t + 1], tensors[1][t:t + 1], tensors[2])
        host.export_confirmed_inputs(feed.inputs, feed.upto, feed.last, feed.disc)
        spec.receive_host_status(feed.last.clone(), feed.disc.clone())
        spec.run_ticks(feed.upto.clone()[None], feed.inputs)

    compared = 0
    for t in range(ticks):
        if t == T_MOVE:
            assert (sc.frames()[0][dst] != sb.frames()[0][sel]).any()
            G.move_sessions(hb, sel, hc, dst)
            G.move_sessions(sb, sel, sc, dst)
            assert hc.import_refused() == 0 and sc.import_refused() == 0
            fc.inputs[:, :, idst] = fb.inputs[:, :, isel]  # the feed's columns move with the pair
            fc.upto[idst] = fb.upto[isel]
            fc.last[:, idst] = fb.last[:, isel]
            fc.disc[:, idst] = fb.disc[:, isel]
            np.testing.assert_array_equal(hc.export_status()[1][dst], hb.export_status()[1][sel])
        tick(hb, sb, fb, dx, t)
        tick(hc, sc, fc, dz if t >= T_MOVE else dy, t)
        if t >= T_MOVE - 1:
            cur, recv = sc.frames()
            if t >= T_MOVE:  # the moved spectators against the ones that stayed, which play on with their hosts
                for x, y in zip(sc.frames() + sc.status() + sc.read_live(), sb.frames() + sb.status() + sb.read_live()):
                    np.testing.assert_array_equal(x[dst], y[sel], err_msg=f"tick {t}")
            img, cs = sc.read_live()
            tags, himg, hcs = hc.read_cells()
            conf = hc.frames()[1]
            for s in (dst if t >= T_MOVE else range(S)):
                f = int(cur[s]) + 1
                if tags[f % W_, s] == f and f <= conf[s]:
                    assert np.array_equal(img[s], himg[f % W_, s]) and np.array_equal(cs[s], hcs[f % W_, s]), f"tick {t} session {s}"
                    compared += t >= T_MOVE
    assert compared > 5 * len(dst), compared
    assert (hc.export_status()[0] == L.RB_P2P_EXPORT_OK).all() and hc.counters()[2] == 0
    assert (sc.frames()[0][dst] > T_MOVE).all()
    for s in (hb, hc, sb, sc):
        s.close()


# ---------------------------------------------------------------------------
# GPU 9: refusals, validation, no-ops, user streams
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_records_of_another_configuration_are_refused(gpu_available):
    import torch
    P, mask, d, rd, ticks = 2, 0b01, 1, 1, 20
    X = network(12, P, mask, rd, S, ticks)
    dx = dev(*X)

    def other(game=G.Game.EX_GAME, w=W, delay=d, time_sync=True, dtype=np.uint8, imask=0x0F):
        b = (G.SessionBuilder(game, num_sessions=S).with_num_players(P).with_max_prediction_window(w)
             .with_input_delay(delay).with_remote_input_delay(rd))
        for h in range(P):
            b.add_player(PlayerType.Local if (mask >> h) & 1 else PlayerType.Remote, h)
        s = b.start_p2p_session()
        if time_sync:
            s.enable_time_sync(60)
        s.run_ticks(*dev(*network(12, P, mask, rd, S, ticks, dtype, imask)))
        return s

    dest, good = other(), other()
    dest.run_ticks(dx[0][:5], dx[1][:5], dx[2])  # 25 ticks: apart from `good`
    foreign = {"another W": other(w=9), "another game": other(game=G.Game.STUB, dtype=np.uint32, imask=0x3),
               "time sync off": other(time_sync=False), "another input delay": other(delay=2)}
    rb = dest.record_bytes
    assert good.record_bytes == rb == foreign["another input delay"].record_bytes
    assert {s.record_bytes for s in foreign.values()} > {rb}, "some foreign records have another size, one has ours"
    rows = [good.export_sessions([7])]
    for s in foreign.values():  # a foreign record, cut or padded to our size: its header says what it is
        r = s.export_sessions([7])
        row = torch.zeros((1, rb), dtype=torch.uint8, device="cuda")
        k = min(rb, r.shape[1])
        row[:, :k] = r[:, :k]
        rows.append(row)
    rows.append(torch.zeros((1, rb), dtype=torch.uint8, device="cuda"))  # no record at all
    rows.append(good.export_sessions([9]))
    records = torch.cat(rows)
    where = np.array([3, 10, 64, 65, 69, 30, 0], np.int32)
    before = everything(dest, True)
    dest.import_sessions(where, records)
    assert dest.import_refused() == len(foreign) + 1
    after = everything(dest, True)
    kept = others(S, where[[0, -1]])
    assert_columns(after, kept, before, kept, "refused records and unselected sessions: bit-identical")
    assert_columns(after, where[[0, -1]], everything(good, True), np.array([7, 9]), "the valid records of the same call")
    np.testing.assert_array_equal(after["totals"], before["totals"])
    np.testing.assert_array_equal(after["counters"], before["counters"])
    dest.import_sessions([1], good.export_sessions([1]))
    assert dest.import_refused() == len(foreign) + 1, "the count is since create and only counts refusals"
    for s in (dest, good, *foreign.values()):
        s.close()


@pytest.mark.gpu
def test_gpu_bad_lists_empty_lists_and_user_streams(gpu_available):
    import torch
    from test_spectator import start_spectators
    P, mask, d, rd = 2, 0b01, 1, 1
    X = network(13, P, mask, rd, S, 40)
    dx = dev(*X)
    b, c, twin = (make_session(G.Game.EX_GAME, P, mask, d, rd) for _ in range(3))
    assert b.import_refused() == 0  # before any import
    for s in (b, c, twin):
        s.run_ticks(dx[0][:20], dx[1][:20], dx[2])
    spec = start_spectators(G.Game.EX_GAME, P, S)
    records = b.export_sessions([0, 1, 2])
    for sess in (b, spec):
        ok = sess.export_sessions([0, 1, 2])
        for bad in ([0, 0, 1], [0, 1, S], [-1, 1, 2]):
            with pytest.raises(G.InvalidRequest, match="distinct indices"):
                sess.export_sessions(bad)
            with pytest.raises(G.InvalidRequest, match="distinct indices"):
                sess.import_sessions(bad, ok)
        with pytest.raises(ValueError):
            sess.import_sessions([0, 1], ok)
        empty = sess.export_sessions([])
        assert tuple(empty.shape) == (0, sess.record_bytes)
        sess.import_sessions([], empty)
        assert sess.import_refused() == 0
    with pytest.raises(ValueError):
        spec.import_sessions([0, 1, 2], records)  # a host's records are not a spectator's size
    want = everything(twin, True)
    # a batch that never paced or exported reads back as before although a move made those rows
    assert (b.parked_ticks() == 0).all() and (b.export_status()[1] == 0).all()
    for k, v in everything(b, True).items():
        np.testing.assert_array_equal(v, want[k], err_msg=f"{k}: refused calls launch nothing, export only reads")
    # on a user stream: the move is ordered between the ticks around it
    stream = torch.cuda.Stream()
    for s in (b, c):
        s.set_stream(stream)
    sel, dst = np.array([5, 64, 69, 2], np.int32), np.array([64, 1, 5, 33], np.int32)
    with torch.cuda.stream(stream):
        b.run_ticks(dx[0][20:30], dx[1][20:30], dx[2])
        G.move_sessions(b, sel, c, dst)
        Z = moved_tensors(tuple(x[10:] if i < 2 else x for i, x in enumerate(X)), tuple(x[:30] if i < 2 else x for i, x in enumerate(X)), sel, dst)
        dz = dev(*Z)
        c.run_ticks(dz[0][20:30], dz[1][20:30], dz[2])
    first = make_session(G.Game.EX_GAME, P, mask, d, rd)
    first.run_ticks(dx[0][:20], dx[1][:20], dx[2])
    for t0 in (20, 30):  # the launches of the moved sessions, and of their new neighbours
        twin.run_ticks(dx[0][t0:t0 + 10], dx[1][t0:t0 + 10], dx[2])
    first.run_ticks(dx[0][20:30], dx[1][20:30], dx[2])
    ec = everything(c, True)
    assert_columns(ec, dst, everything(twin, True), sel, "user stream, moved: 40 ticks of X")
    assert_columns(ec, others(S, dst), everything(first, True), others(S, dst), "user stream, neighbours: 30 ticks of X")
    for s in (b, c, twin, first, spec):
        s.close()
