"""SpectatorSession batches (ggrs_amd/csrc/spectator.hpp) and the host's
confirmed-input feed (rb_p2p_export_confirmed_inputs).

oracle/ has no spectator, so this file carries a Python restatement of
SpectatorSession::advance_frame / inputs_at_frame / Event::Input
(sessions/p2p_spectator_session.rs:109-139, 173-202, 233-237) with the explicit
60-slot ring (``SpectatorModel``).  The expected game states come from the
existing OracleP2P: a "truth" run in which every input is delivered before it
is needed saves the cell of frame f holding the state after frames 0..f-1,
which is the state a spectator has after its frame f-1 (the pattern of
test_p2p.py:81-92).
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import ggrs_amd as G
from ggrs_amd import _lib as L
from ggrs_amd.p2p import PlayerType, synth_network
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, THRESHOLD, TOO_FAR = L.RB_OK, L.RB_PREDICTION_THRESHOLD, L.RB_SPECTATOR_TOO_FAR_BEHIND
BUFFER = 60  # SPECTATOR_BUFFER_SIZE (p2p_spectator_session.rs:16)
ORC_GAME = {G.Game.EX_GAME: O.EX_GAME, G.Game.STUB: O.STUB, G.Game.STUB_ENUM: O.STUB_ENUM, G.Game.BRAWLER: O.BRAWLER}


# ---------------------------------------------------------------------------- the model
class SpectatorModel:
    """One SpectatorSession's frame bookkeeping, restated line by line (Running from the start)."""

    def __init__(self, max_frames_behind=10, catchup_speed=1):  # builder.rs:23-25
        self.ring = [G.NULL_FRAME] * BUFFER  # inputs[slot][0].frame: blank_input(NULL_FRAME) (:59-62)
        self.current_frame = G.NULL_FRAME  # :67
        self.last_recv_frame = G.NULL_FRAME  # :68
        self.max_frames_behind, self.catchup_speed = max_frames_behind, catchup_speed

    def deliver(self, upto):
        """Event::Input for every frame after last_recv_frame up to `upto`, in order (:233-237)."""
        for f in range(self.last_recv_frame + 1, upto + 1):
            self.ring[f % BUFFER] = f  # :235
            assert f >= self.last_recv_frame  # :236
            self.last_recv_frame = f  # :237

    def frames_behind_host(self):  # :80-84
        diff = self.last_recv_frame - self.current_frame
        assert diff >= 0
        return diff

    def inputs_at_frame(self, frame_to_grab):  # :173-187
        tag = self.ring[frame_to_grab % BUFFER]
        if tag < frame_to_grab:
            return THRESHOLD
        if tag > frame_to_grab:
            return TOO_FAR
        return OK

    def advance_frame(self):
        """(status, AdvanceFrame requests built, frames current_frame moved) (:119-138)."""
        n = self.catchup_speed if self.frames_behind_host() > self.max_frames_behind else 1  # :119-123
        moved = 0
        for _ in range(n):  # :125-136
            st = self.inputs_at_frame(self.current_frame + 1)
            if st != OK:
                return st, 0, moved  # `?`: the requests built so far are dropped
            self.current_frame += 1
            moved += 1
        return OK, n, moved


def rule_status(last_recv, f):
    """The kernel's implicit ring (spectator.hpp): decided by last_recv alone."""
    return THRESHOLD if last_recv < f else (TOO_FAR if last_recv >= f + BUFFER else OK)


def run_model(upto, max_behind, catchup):
    """Per tick and session (status, n_advance, current, last_recv) of the model, [T, S, 4]."""
    T, S = upto.shape
    models = [SpectatorModel(max_behind, catchup) for _ in range(S)]
    out = np.empty((T, S, 4), np.int32)
    for t in range(T):
        for s, m in enumerate(models):
            m.deliver(int(upto[t, s]))
            st, n, moved = m.advance_frame()
            assert moved == (n if st == OK else 0), "the partial-progress path (:125-136) must be unreachable"
            out[t, s] = (st, n, m.current_frame, m.last_recv_frame)
    return out


# ---------------------------------------------------------------------------- CPU
MSG_BEHIND_SMALL = "Max frames behind cannot be smaller than 1."
MSG_BEHIND_LARGE = "Max frames behind cannot be larger or equal than the Spectator buffer size (60)"
MSG_SPEED_SMALL = "Catchup speed cannot be smaller than 1."
MSG_SPEED_LARGE = "Catchup speed cannot be larger or equal than the allowed maximum frames behind host"


def test_builder_validation_messages_and_order():
    # builder.rs:210-244: each setter checks against the builder's state at that call
    b = lambda: G.SessionBuilder(G.Game.EX_GAME, num_sessions=4)
    for call, msg in [(lambda: b().with_max_frames_behind(0), MSG_BEHIND_SMALL),
                      (lambda: b().with_max_frames_behind(60), MSG_BEHIND_LARGE),
                      (lambda: b().with_catchup_speed(0), MSG_SPEED_SMALL),
                      (lambda: b().with_catchup_speed(10), MSG_SPEED_LARGE),  # the default max_frames_behind is 10
                      (lambda: b().with_max_frames_behind(3).with_catchup_speed(3), MSG_SPEED_LARGE)]:
        with pytest.raises(G.InvalidRequest) as e:
            call()
        assert e.value.info == msg
    # accepted: the defaults' values, the largest values, and a speed checked against a raised limit
    b().with_max_frames_behind(10).with_catchup_speed(1)
    b().with_max_frames_behind(59).with_catchup_speed(58)
    # order dependent like the reference: the speed was valid when it was set ...
    late = b().with_catchup_speed(5).with_max_frames_behind(4)
    with pytest.raises(G.InvalidRequest) as e:  # ... and the create call checks the final values
        late.start_spectator_session()
    assert e.value.info == MSG_SPEED_LARGE


def _create(**kw):
    lib = L.load()
    cfg = L.RbSpectatorConfig()
    lib.rb_spectator_config_init(ctypes.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    st = lib.rb_spectator_create(ctypes.byref(cfg), ctypes.byref(h))
    msg = (lib.rb_spectator_last_error(None) or b"").decode()
    if h:
        lib.rb_spectator_destroy(h)
    return st, msg, cfg


def test_create_validation_before_any_device_work():
    for kw, msg in [({"max_frames_behind": 0}, MSG_BEHIND_SMALL), ({"max_frames_behind": 60}, MSG_BEHIND_LARGE),
                    ({"catchup_speed": 0}, MSG_SPEED_SMALL), ({"catchup_speed": 10}, MSG_SPEED_LARGE),
                    ({"max_frames_behind": 4, "catchup_speed": 4}, MSG_SPEED_LARGE)]:
        st, got, _ = _create(**kw)
        assert st == L.RB_INVALID_REQUEST and got == msg
    # the game and player-count rules of rb_p2p_create
    assert _create(num_players=5)[0] == L.RB_INVALID_REQUEST
    assert _create(game=L.RB_GAME_STUB_RANDOM_CS)[0] == L.RB_INVALID_REQUEST
    assert _create(game=L.RB_GAME_STUB, num_players=3)[0] == L.RB_INVALID_REQUEST
    # the defaults (builder.rs:13, 23-25) pass validation: OK with a GPU, a device error without one
    st, _, cfg = _create()
    assert (cfg.num_players, cfg.max_frames_behind, cfg.catchup_speed) == (2, 10, 1)
    assert st in (L.RB_OK, L.RB_DEVICE_ERROR)


def test_model_prediction_threshold_before_any_input():
    m = SpectatorModel()
    assert m.frames_behind_host() == 0
    assert m.advance_frame() == (THRESHOLD, 0, 0) and m.current_frame == G.NULL_FRAME
    m.deliver(0)
    assert m.frames_behind_host() == 1
    assert m.advance_frame() == (OK, 1, 1) and m.current_frame == 0 and m.frames_behind_host() == 0
    assert m.advance_frame() == (THRESHOLD, 0, 0) and m.current_frame == 0


def test_model_catches_up_at_catchup_speed():
    m = SpectatorModel(max_frames_behind=5, catchup_speed=3)
    m.deliver(20)
    steps = []
    while m.frames_behind_host() > 0:
        st, n, moved = m.advance_frame()
        assert st == OK and moved == n
        steps.append(n)
    # 21 behind: 3 per tick while more than 5 behind (21, 18, 15, 12, 9, 6), then 1 per tick
    assert steps == [3] * 6 + [1] * 3 and m.current_frame == 20


def test_model_too_far_behind_exactly_from_61_frames():
    for ahead, want in [(59, OK), (60, OK), (61, TOO_FAR), (100, TOO_FAR)]:
        m = SpectatorModel()
        m.deliver(9)
        for _ in range(10):
            assert m.advance_frame()[0] == OK
        assert m.current_frame == 9
        m.deliver(9 + ahead)
        assert m.frames_behind_host() == ahead
        st, n, moved = m.advance_frame()
        assert st == want and moved == (1 if want == OK else 0)
        if want == TOO_FAR:  # the input is gone for good: no later delivery helps
            m.deliver(9 + ahead + 30)
            assert m.advance_frame() == (TOO_FAR, 0, 0) and m.current_frame == 9


def test_model_ring_equals_the_last_recv_rule_on_random_contiguous_deliveries():
    rng = np.random.default_rng(5)
    for trial in range(40):
        mb = int(rng.integers(2, 60))  # catchup_speed < max_frames_behind < 60 (builder.rs:210-244)
        m = SpectatorModel(mb, int(rng.integers(1, mb)))
        errors = 0
        for t in range(300):
            jump = int(rng.choice([0, 0, 1, 1, 1, 2, 7, 30, 70]))
            m.deliver(m.last_recv_frame + jump)
            # every frame, not only the one the next tick asks for
            for f in range(max(0, m.current_frame - 2), m.current_frame + 70):
                assert m.inputs_at_frame(f) == rule_status(m.last_recv_frame, f)
            want = rule_status(m.last_recv_frame, m.current_frame + 1)
            st, n, moved = m.advance_frame()
            assert st == want and moved == (n if st == OK else 0)
            errors += st != OK
        assert errors > 0


# ---------------------------------------------------------------------------- shared inputs, schedule and truth
S_, T_, F_ = 70, 90, 104  # sessions (the last wave is partial), ticks, frames of the input tensors
MAX_BEHIND, CATCHUP = 5, 3


def schedule(S=S_, T=T_):
    """host_upto [T, S]: by session % 5 — 0 starves (a frame every other tick), 1 is fed every tick
    (never an error), 2 stalls twice for 15 ticks and then receives a burst (catch-up), 3 jumps 70
    frames ahead at tick 30 (TooFarBehind from then on), 4 jumps exactly 60 ahead at tick 40 (the
    last distance that is not an error) and then starves once it has caught up."""
    t = np.arange(T, dtype=np.int32)
    rows = [t // 2 - 1,
            t,
            np.where(t < 20, t, np.where(t < 35, 19, np.where(t < 55, t, np.where(t < 70, 54, t)))),
            np.where(t < 30, t, 100),
            np.where(t < 40, t, 99)]
    return np.stack([rows[s % 5] for s in range(S)], axis=1).astype(np.int32)


def test_schedule_covers_every_path_on_the_model():
    m = run_model(schedule(), MAX_BEHIND, CATCHUP)
    st, n = m[:, :, 0], m[:, :, 1]
    assert (n > 1).sum() > S_, "more than S catch-up ticks"
    assert (st == THRESHOLD).any(axis=0).sum() >= 1 and (st == TOO_FAR).any(axis=0).sum() >= 1
    assert (st == OK).all(axis=0).sum() >= 1, "a session that is never in error"
    behind_before = m[:, :, 3] - (m[:, :, 2] - n)  # frames_behind_host when the tick began
    assert behind_before[st == OK].max() == BUFFER, "60 behind and still advancing"
    assert behind_before[st == TOO_FAR].min() == BUFFER + 11
    far = (st == TOO_FAR).any(axis=0)
    first = (st[:, far] == TOO_FAR).argmax(axis=0)
    for k, s in enumerate(np.nonzero(far)[0]):  # frozen from the first error on
        assert (st[first[k]:, s] == TOO_FAR).all() and (m[first[k]:, s, 2] == m[first[k], s, 2]).all()
    assert m[:, :, 3].max() < F_ - 1


def game_inputs(game, P, S, F, seed=11):
    dt = np.uint32 if game == G.Game.STUB else np.uint8
    mask = {G.Game.STUB: 0x3, G.Game.STUB_ENUM: 0x1, G.Game.EX_GAME: 0x0F}.get(game, 0x1F)
    return G.synth_inputs(S, P, F, seed=seed, mask=mask, dtype=dt)


def truth_cells(orc_game, P, X, disc=None, lib_path=None):
    """seen[(s, f)] = (image, checksum) of the frame-f cell of a P2P run over the inputs X[f, p, s]
    by frame in which nothing is predicted: player 0 local without delay, the others remote and
    delivered ahead.  disc = (handle, last [S], sel [S]): in the selected sessions the handle's
    inputs end at frame last[s] and it is disconnected before the first tick, so every later frame
    advances with (zeroed, Disconnected) (test_p2p.py:166-193, without the late deliveries)."""
    F, _, S = X.shape
    kw = {} if lib_path is None else {"lib_path": lib_path}
    orc = O.OracleP2P(orc_game, P, 8, 0, 0b01, S, remote_delay=0, **kw)
    seen = {}
    for t in range(F):
        for h in range(1, P):
            up = np.full(S, min(t + 4, F - 1), np.int32)
            if disc is not None and h == disc[0]:
                up = np.where(disc[2], disc[1], up).astype(np.int32)
            assert orc.deliver(h, up, X[:, h, :]) == 0, orc.last_panic()
        if t == 0 and disc is not None:
            assert orc.disconnect_player(disc[0], disc[2]) == 0
        assert orc.add_local_input(0, X[t, 0]) == 0
        st, lf, _, _ = orc.advance()
        assert (st == 0).all() and (lf == G.NULL_FRAME).all(), orc.last_panic()
        tags, imgs, cs = orc.read_cells()
        for w in range(tags.shape[0]):
            for s in range(S):
                if tags[w, s] >= 0 and (s, int(tags[w, s])) not in seen:
                    seen[(s, int(tags[w, s]))] = (imgs[w, s].copy(), cs[w, s].copy())
    orc.close()
    return seen


@functools.lru_cache(maxsize=None)
def shared_case(game, P, S):
    """(inputs X [F, P, S], truth cells) of one game and shape, computed once and only read."""
    X = game_inputs(game, P, S, F_)
    X.setflags(write=False)
    return X, truth_cells(ORC_GAME[game], P, X)


def assert_state_is_truth(sess, seen, note):
    """The spectator's image and checksum are those of the truth's cell of frame current + 1."""
    cur, _ = sess.frames()
    img, cs = sess.read_live()
    for s in range(sess.num_sessions):
        timg, tcs = seen[(s, int(cur[s]) + 1)]
        assert np.array_equal(img[s], timg), f"{note}: session {s} state after frame {cur[s]}"
        assert np.array_equal(cs[s], tcs), f"{note}: session {s} checksum of frame {cur[s] + 1}"


def start_spectators(game, P, S, max_behind=MAX_BEHIND, catchup=CATCHUP):
    return (G.SessionBuilder(game, num_sessions=S).with_num_players(P).with_max_frames_behind(max_behind)
            .with_catchup_speed(catchup).start_spectator_session())


def run_schedule_every_tick(sess, upto, X, seen):
    """One-tick launches of the schedule; status, counts and frames against the model and the
    state against the truth after every tick."""
    import torch
    model = run_model(upto, sess.max_frames_behind, sess.catchup_speed)
    du, dx = torch.from_numpy(upto).cuda(), torch.from_numpy(X.copy()).cuda()
    for t in range(upto.shape[0]):
        sess.run_ticks(du[t:t + 1], dx)
        st, na = sess.status()
        cur, recv = sess.frames()
        for k, got in enumerate((st, na, cur, recv)):
            np.testing.assert_array_equal(got, model[t, :, k], err_msg=f"tick {t}, field {k}")
        np.testing.assert_array_equal(sess.frames_behind_host(), model[t, :, 3] - model[t, :, 2])
        assert_state_is_truth(sess, seen, f"tick {t}")
    st = model[:, :, 0]
    assert sess.totals() == (int(model[:, :, 1].sum()), int((st == THRESHOLD).sum()), int((st == TOO_FAR).sum()))
    return model


# ---------------------------------------------------------------------------- GPU
SPECTATOR_CASES = [(G.Game.EX_GAME, 2, S_), (G.Game.EX_GAME, 3, S_), (G.Game.EX_GAME, 4, S_), (G.Game.STUB, 2, S_),
                   (G.Game.STUB_ENUM, 2, S_), (G.Game.BRAWLER, 2, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("game,P,S", SPECTATOR_CASES, ids=[f"{g.name}-P{p}-S{s}" for g, p, s in SPECTATOR_CASES])
def test_gpu_spectator_matches_model_and_truth_every_tick(gpu_available, game, P, S):
    X, seen = shared_case(game, P, S)
    upto = schedule(S)
    sess = start_spectators(game, P, S)
    assert sess.num_players() == P and sess.state_bytes == len(seen[(0, 0)][0])
    c0, r0 = sess.frames()
    assert (c0 == G.NULL_FRAME).all() and (r0 == G.NULL_FRAME).all()  # :67-68
    model = run_schedule_every_tick(sess, upto, X, seen)
    st, n = model[:, :, 0], model[:, :, 1]
    if S == S_:  # the coverage the schedule was chosen for (the brawler's 5 sessions hold one of each kind)
        assert (n > 1).sum() > S
    assert (st == THRESHOLD).any() and (st == TOO_FAR).any() and (st == OK).all(axis=0).any()
    sess.close()


@pytest.mark.gpu
@pytest.mark.parametrize("game,P", [(G.Game.EX_GAME, 2), (G.Game.EX_GAME, 3), (G.Game.STUB, 2)])
def test_gpu_spectator_fused_launches_equal_one_tick_launches(gpu_available, game, P):
    import torch
    X, seen = shared_case(game, P, S_)
    upto = schedule()
    du, dx = torch.from_numpy(upto).cuda(), torch.from_numpy(X.copy()).cuda()
    results = []
    for chunk in (1, 7, 90):
        sess = start_spectators(game, P, S_)
        for t in range(0, T_, chunk):
            sess.run_ticks(du[t:t + chunk], dx)
        results.append((sess.read_live(), sess.frames(), sess.status(), sess.totals()))
        assert_state_is_truth(sess, seen, f"launches of {chunk}")
        sess.close()
    for other in results[1:]:
        for a, b in zip(results[0], other):
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("game,P,h", [(G.Game.EX_GAME, 3, 2), (G.Game.STUB, 2, 1), (G.Game.BRAWLER, 2, 1)])
def test_gpu_spectator_disconnected_status(gpu_available, game, P, h):
    # host_connect_status marks handle h disconnected at last_frame = L in a third of the sessions:
    # frames past L advance with (zeroed, Disconnected) (:193-199), like a P2P session that
    # disconnected the player at that frame
    import torch
    S = 5 if game == G.Game.BRAWLER else S_
    sel = np.arange(S) % 3 == 1
    last = (12 + np.arange(S) % 7).astype(np.int32)
    X0 = game_inputs(game, P, S, F_, seed=23)
    X = X0.copy()
    for s in np.nonzero(sel)[0]:
        X[last[s] + 1:, h, s] = 0  # what the host sends for them (sync_layer.rs:210-211)
    seen = truth_cells(ORC_GAME[game], P, X, disc=(h, last, sel))
    plain = truth_cells(ORC_GAME[game], P, X0)  # the player stays connected and goes on sending
    s0 = int(np.nonzero(sel)[0][0])
    assert not np.array_equal(seen[(s0, 40)][0], plain[(s0, 40)][0]), "the disconnect must change the game"
    sess = start_spectators(game, P, S)
    lf = np.full((P, S), G.NULL_FRAME, np.int32)
    dc = np.zeros((P, S), np.uint8)
    lf[h, sel], dc[h, sel] = last[sel], 1
    sess.receive_host_status(torch.from_numpy(lf).cuda(), torch.from_numpy(dc).cuda())
    # the merge (protocol.rs:629-636): an older report changes nothing
    sess.receive_host_status(torch.from_numpy(np.minimum(lf, 3)).cuda(), torch.zeros((P, S), dtype=torch.uint8).cuda())
    upto = np.minimum(np.arange(T_, dtype=np.int32)[:, None] + (np.arange(S) % 3)[None, :], F_ - 2).astype(np.int32)
    dx = torch.from_numpy(X).cuda()
    du = torch.from_numpy(upto).cuda()
    for t in range(0, T_, 9):
        sess.run_ticks(du[t:t + 9], dx)
        assert_state_is_truth(sess, seen, f"tick {t + 8}")
    cur, _ = sess.frames()
    assert (cur == T_ - 1).all() and (sess.status()[0] == OK).all()
    sess.close()


# -- the host's export
HOST_CASES = [  # game, P, local mask, sparse saving, (tick, handle) of a disconnect_player or None
    (G.Game.EX_GAME, 2, 0b01, False, None),
    (G.Game.EX_GAME, 4, 0b0101, False, None),
    (G.Game.STUB, 2, 0b10, False, None),
    (G.Game.EX_GAME, 2, 0b01, False, (40, 1)),
    (G.Game.EX_GAME, 2, 0b01, True, None),
]
HOST_IDS = [f"{c[0].name}-P{c[1]}-m{c[2]}-sp{int(c[3])}-{'disc' if c[4] else 'conn'}" for c in HOST_CASES]
DELAY, REMOTE_DELAY, W_ = 2, 1, 8


def start_host(game, P, mask, S, sparse=False):
    b = (G.SessionBuilder(game, num_sessions=S).with_num_players(P).with_max_prediction_window(W_)
         .with_input_delay(DELAY).with_remote_input_delay(REMOTE_DELAY).with_sparse_saving_mode(sparse))
    for h in range(P):
        b.add_player(PlayerType.Local if (mask >> h) & 1 else PlayerType.Remote, h)
    return b.start_p2p_session()


def host_network(game, P, mask, S, T):
    dt = np.uint32 if game == G.Game.STUB else np.uint8
    imask = {G.Game.STUB: 0x3, G.Game.STUB_ENUM: 0x1}.get(game, 0x0F)
    return synth_network(S, P, T, mask, REMOTE_DELAY, 1, 5, dtype=dt, mask=imask)


class Feed:
    """The device tensors of one host's export, prefilled with a sentinel."""

    def __init__(self, sess, frames):
        import torch
        P, S = sess.num_players, sess.num_sessions
        tdt = torch.int32 if np.dtype(sess.input_dtype).itemsize == 4 else torch.uint8
        self.sentinel = 0x5A5A5A5A if tdt == torch.int32 else 0x5A
        self.inputs = torch.full((frames, P, S), self.sentinel, dtype=tdt, device="cuda")
        self.upto = torch.full((S,), -7, dtype=torch.int32, device="cuda")
        self.last = torch.full((P, S), -7, dtype=torch.int32, device="cuda")
        self.disc = torch.full((P, S), 9, dtype=torch.uint8, device="cuda")
        self.sess = sess

    def export(self):
        self.sess.export_confirmed_inputs(self.inputs, self.upto, self.last, self.disc)
        return (self.inputs.cpu().numpy().view(self.sess.input_dtype), self.upto.cpu().numpy(),
                self.last.cpu().numpy(), self.disc.cpu().numpy())


def expected_by_frame(P, mask, inputs, rin, frames):
    """Every player's confirmed input by frame: a remote player's delivered input, a local
    player's input delayed by the input delay (frames below the delay are not checked)."""
    S = inputs.shape[2]
    want = np.zeros((frames, P, S), inputs.dtype)
    known = np.zeros((frames, P), bool)
    for h in range(P):
        if (mask >> h) & 1:
            n = min(frames - DELAY, inputs.shape[0])
            want[DELAY:DELAY + n, h] = inputs[:n, h]
            known[DELAY:DELAY + n, h] = True
        else:
            n = min(frames, rin.shape[0])
            want[:n, h] = rin[:n, h]
            known[:n, h] = True
    return want, known


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [1, 13])
@pytest.mark.parametrize("case", HOST_CASES[:4], ids=HOST_IDS[:4])
def test_gpu_export_against_the_host(gpu_available, case, chunk):
    import torch
    game, P, mask, sparse, disc = case
    S, T = S_, T_ + 1  # 91 = 7 launches of 13
    inputs, upto, rin = host_network(game, P, mask, S, T)
    host = start_host(game, P, mask, S, sparse)
    di, du, dr = (torch.from_numpy(a).cuda() for a in (inputs, upto, rin))
    F = T + DELAY + 4
    feed = Feed(host, F)
    want, known = expected_by_frame(P, mask, inputs, rin, F)
    prev = np.full(S, G.NULL_FRAME, np.int32)
    disc_last = None
    for t in range(0, T, chunk):
        if disc and t <= disc[0] < t + chunk:
            # between launches: at the launch that holds the tick (chunk 13: tick 39, chunk 1: tick 40)
            host.disconnect_player(disc[1])
            disc_last = host.read_queues()[:, disc[1], 6].copy()
        host.run_ticks(di[t:t + chunk], du[t:t + chunk], dr)
        got, gup, glast, gdisc = feed.export()
        q = host.read_queues()
        conn, dflag = q[:, :, 6], q[:, :, 7] != 0
        confirmed = np.where(dflag, np.iinfo(np.int32).max, conn).min(axis=1)  # p2p_session.rs:487-498
        np.testing.assert_array_equal(gup, confirmed, err_msg=f"tick {t}")
        assert (gup >= prev).all()
        prev = gup
        np.testing.assert_array_equal(glast, conn.T)
        np.testing.assert_array_equal(gdisc != 0, dflag.T)
        for s in range(S):
            u = int(gup[s])
            assert (got[u + 1:, :, s] == feed.sentinel).all(), f"session {s}: written past upto"
            for h in range(P):
                k = known[:u + 1, h]
                w = want[:u + 1, h, s].copy()
                if disc_last is not None and h == disc[1]:
                    w[disc_last[s] + 1:] = 0  # a disconnected player's later frames
                assert np.array_equal(got[:u + 1, h, s][k], w[k]), f"tick {t} session {s} handle {h}"
    assert (host.export_status()[0] == L.RB_P2P_EXPORT_OK).all()
    assert (host.export_status()[1] == prev + 1).all()
    assert prev.min() > 60
    if disc:
        assert (prev > disc_last + 20).all(), "frames past the disconnect were exported"
    host.close()


def host_truth(game, P, mask, inputs, rin, T, disc=None, disc_last=None):
    """The cells of the host's own configuration with every remote input delivered ahead
    (test_p2p.py:81-92); disc: the handle is disconnected before the first tick with its inputs
    ending at disc_last[s]."""
    S = inputs.shape[2]
    orc = O.OracleP2P(ORC_GAME[game], P, W_, DELAY, mask, S, remote_delay=REMOTE_DELAY)
    seen = {}
    for t in range(T):
        for h in range(P):
            if not (mask >> h) & 1:
                up = np.full(S, min(t + 4 + REMOTE_DELAY, rin.shape[0] - 1), np.int32)
                if disc is not None and h == disc:
                    up = disc_last.astype(np.int32)
                assert orc.deliver(h, up, rin[:, h, :]) == 0, orc.last_panic()
        if t == 0 and disc is not None:
            assert orc.disconnect_player(disc) == 0
        for h in range(P):
            if (mask >> h) & 1:
                assert orc.add_local_input(h, inputs[t, h]) == 0
        st, lf, _, _ = orc.advance()
        assert (st == 0).all() and (lf == G.NULL_FRAME).all(), orc.last_panic()
        tags, imgs, cs = orc.read_cells()
        for w in range(tags.shape[0]):
            for s in range(S):
                if tags[w, s] >= 0 and (s, int(tags[w, s])) not in seen:
                    seen[(s, int(tags[w, s]))] = (imgs[w, s].copy(), cs[w, s].copy())
    orc.close()
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("case", HOST_CASES, ids=HOST_IDS)
def test_gpu_host_feeds_spectators_end_to_end(gpu_available, case):
    import torch
    game, P, mask, sparse, disc = case
    S, T = S_, T_
    # (8 more ticks of inputs than the host runs: after a disconnect the confirmed frame runs ahead
    # of the host's current frame, and the truth must reach every frame a spectator can)
    inputs, upto, rin = host_network(game, P, mask, S, T + 8)
    host = start_host(game, P, mask, S, sparse)
    spec = start_spectators(game, P, S)
    di, du, dr = (torch.from_numpy(a).cuda() for a in (inputs, upto, rin))
    feed = Feed(host, T + DELAY + 4)
    seen = None if disc else host_truth(game, P, mask, inputs, rin, T + 8)
    delay = torch.from_numpy((np.arange(S) % 4).astype(np.int64)).cuda()  # the feed reaches session s delay[s] ticks late
    history = torch.full((T + 4, S), G.NULL_FRAME, dtype=torch.int32, device="cuda")
    ar = torch.arange(S, device="cuda")
    disc_last, compared_host = None, 0

    def check(t):
        nonlocal compared_host
        assert_state_is_truth(spec, seen, f"tick {t}")
        cur, _ = spec.frames()
        img, cs = spec.read_live()
        tags, himg, hcs = host.read_cells()
        _, conf = host.frames()
        for s in range(S):  # the host's own cell of frame current + 1, once confirmed: another kernel, the same bits
            f = int(cur[s]) + 1
            w = f % W_
            if tags[w, s] == f and f <= conf[s]:
                assert np.array_equal(img[s], himg[w, s]) and np.array_equal(cs[s], hcs[w, s]), f"tick {t} session {s}"
                compared_host += 1

    for t in range(T):
        if disc and t == disc[0]:
            host.disconnect_player(disc[1])
            disc_last = host.read_queues()[:, disc[1], 6].copy()
            seen = host_truth(game, P, mask, inputs, rin, T + 8, disc=disc[1], disc_last=disc_last)
        host.run_ticks(di[t:t + 1], du[t:t + 1], dr)
        host.export_confirmed_inputs(feed.inputs, feed.upto, feed.last, feed.disc)
        history[t + 3] = feed.upto
        # (copies: the next export rewrites the status tensors while this tick may still read them;
        # the input tensor only grows, frames a spectator reads are never rewritten)
        spec.receive_host_status(feed.last.clone(), feed.disc.clone())
        spec.run_ticks(history[t + 3 - delay, ar][None].contiguous(), feed.inputs)
        if t % 10 == 9 and seen is not None:
            check(t)
    check(T - 1)
    cur, recv = spec.frames()
    assert cur.min() > 60 and (recv >= cur).all()
    assert compared_host > 0 or sparse
    adv, thr, far = spec.totals()
    assert adv == int((cur + 1).sum()) and far == 0
    host.close()
    spec.close()


@pytest.mark.gpu
def test_gpu_export_overwrite_rule(gpu_available):
    # A host that runs 140 ticks before its first export has overwritten input-ring slots of
    # frames it still had to send: those sessions report RB_P2P_EXPORT_OVERRUN and export nothing,
    # now or later.  Sessions whose remote player stopped sending at frame 50 stalled below 128
    # frames and export as usual.  A status path: no panic, the ticks are untouched.
    import torch
    game, P, mask, S, T = G.Game.EX_GAME, 2, 0b01, S_, 150
    inputs, upto, rin = host_network(game, P, mask, S, T)
    stalled = np.arange(S) % 3 == 0
    upto[:, 1, stalled] = np.minimum(upto[:, 1, stalled], 50)
    host = start_host(game, P, mask, S)
    di, du, dr = (torch.from_numpy(a).cuda() for a in (inputs, upto, rin))
    assert (host.export_status()[0] == L.RB_P2P_EXPORT_OK).all() and (host.export_status()[1] == 0).all()
    host.run_ticks(di[:140], du[:140], dr)
    status_before = host.status()[0].copy()
    feed = Feed(host, T + 8)
    want, known = expected_by_frame(P, mask, inputs, rin, T + 8)
    for step in range(2):
        got, gup, _, _ = feed.export()
        est, nxt = host.export_status()
        np.testing.assert_array_equal(est, np.where(stalled, L.RB_P2P_EXPORT_OK, L.RB_P2P_EXPORT_OVERRUN))
        assert (gup[~stalled] == G.NULL_FRAME).all() and (nxt[~stalled] == 0).all()
        assert (got[:, :, ~stalled] == feed.sentinel).all(), "an overrun session exports nothing"
        assert (gup[stalled] == 50).all()
        for s in np.nonzero(stalled)[0]:
            for h in range(P):
                k = known[:51, h]
                assert np.array_equal(got[:51, h, s][k], want[:51, h, s][k])
            assert (got[51:, :, s] == feed.sentinel).all()
        if step == 0:
            np.testing.assert_array_equal(host.status()[0], status_before)
            host.run_ticks(di[140:], du[140:], dr)  # sticky: later exports change nothing
    assert host.counters()[2] == 0 and (host.status()[0] != L.RB_PANIC).all()
    assert (host.status()[0][stalled] == THRESHOLD).all()
    host.close()


@pytest.mark.gpu
def test_gpu_plugin_game_spectators(gpu_available):
    # the orbit test game (tests/plugin_game/orbit_game.hpp) through the plug-in ABI: the
    # spectator launcher is instantiated in the plug-in's own library
    from ggrs_amd.plugin import register_game_plugin
    plugin = os.path.join(ROOT, "tests", "plugin_game", "libggrs_game_orbit.so")
    lib = ctypes.CDLL(plugin)
    assert lib.rb_plugin_abi() == 8
    gid = register_game_plugin(plugin)
    P = 3
    X = G.synth_inputs(S_, P, F_, seed=7, mask=0x1F)
    seen = truth_cells(O.PLUGIN, P, X, lib_path=O.plugin_lib("orbit"))
    sess = start_spectators(gid, P, S_)
    run_schedule_every_tick(sess, schedule(), X, seen)
    sess.close()
