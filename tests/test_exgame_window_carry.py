"""The prepared window of the fused ex_game SyncTest tick carried from tick to tick (games.hpp
ExGame::extend / carry_ok, kernels.hpp steady_kernel): within a launch only the newest frame's
rotation step, sine/cosine and thrust are computed, the other CD frames move down by one.

What is carried must be what a fresh `prepare` of the loaded cell would give, so how a run of
ticks is cut into launches (every launch starts with a full `prepare`) must not show in any
stored bit.  Every valid cell, the live state and the display checksum are compared with the
oracle after every launch, for three partitions of the same ticks, with inputs pinned so that a
window that slid wrongly (a frame entering or leaving at the wrong position, a wrap on a carried
frame) changes a rotation or a thrust.

(Checked once against a build whose `extend` left frame 2's thrust in place: every one-launch and
mixed case at check distance 7 and 16 failed, 16 of 48.)

Ticks per run: the cd+1 start-up ticks, then max(3 (cd+1) + 10, 82 - (cd+1)) fused ones.  82 ticks
in all is what the slowest pinned property needs: with one player the ship starts at rotation pi
and a constant LEFT (input delay 2: 80 applied frames of 2.5/60 each, 3.33 rad) takes 76 frames to
wrap; a constant thrust passes the speed limit after 42 (v -> 0.98 v + 0.25 exceeds 7).
"""
import numpy as np
import pytest

import ggrs_amd as G
from ggrs_amd.synth import synth_inputs
from oracle import oracle as O

pytestmark = pytest.mark.gpu

S, DELAY = 70, 2  # 70 sessions: a partial last wave for 1, 2 and 4 lanes per session
UP, DOWN, LEFT, RIGHT = 1, 2, 4, 8
PLAYERS = [1, 2, 3, 4]
CDS = [1, 2, 7, 16]


def total_ticks(cd):
    return (cd + 1) + max(3 * (cd + 1) + 10, 82 - (cd + 1))


def pinned_inputs(P, cd):
    """synth_inputs with pinned sessions (every player of a pinned session gets the same byte),
    some in the first wave and some in the partial last one."""
    T = total_ticks(cd)
    inputs = synth_inputs(S, P, T, seed=700 + 10 * P + cd, mask=0x0F)
    t = np.arange(T)
    alt = np.where(t % 2 == 0, LEFT, RIGHT).astype(inputs.dtype)
    llrr = np.where((t // 2) % 2 == 0, LEFT, RIGHT).astype(inputs.dtype)

    def impulse(at):
        v = np.zeros(T, inputs.dtype)
        v[at] = UP | LEFT
        return v

    start = cd + 1  # first fused tick
    pins = {
        0: np.full(T, UP, inputs.dtype), S - 1: np.full(T, UP, inputs.dtype),
        1: np.full(T, UP | LEFT, inputs.dtype), S - 2: np.full(T, UP | LEFT, inputs.dtype),
        2: np.full(T, DOWN | RIGHT, inputs.dtype), S - 3: np.full(T, DOWN | RIGHT, inputs.dtype),
        # the impulse's frame (tick + delay) enters a carried window at position CD and leaves at 0
        3: impulse(start + 3), 4: impulse(start + cd + 4), S - 4: impulse(start + 2 * cd + 5),
        5: alt, S - 5: alt,  # a player that starts at rotation 0 (P = 2, 4) wraps every other tick
        6: llrr, S - 6: llrr,
    }
    for s, v in pins.items():
        inputs[:, :, s] = v[:, None]
    return inputs


_oracle_runs = {}


def oracle_run(P, cd):
    """The oracle's cells and live state after every tick, computed once per (P, cd) and shared by
    the three partitions (never modified)."""
    key = (P, cd)
    if key in _oracle_runs:
        return _oracle_runs[key]
    inputs = pinned_inputs(P, cd)
    orc = O.OracleBatch(O.EX_GAME, P, cd + 1, cd, DELAY, S)
    recs = []
    clamped = wrapped = 0
    prev_rot = None
    for t in range(inputs.shape[0]):
        for h in range(P):
            orc.add_local_input(h, inputs[t, h])
        kinds, _ = orc.advance()
        assert (kinds == 0).all(), orc.last_panic()
        frames, imgs, valid, cs = orc.read_cells()
        live = orc.read_live()
        recs.append((np.array(frames).copy(), np.array(imgs).copy(), np.array(cs).copy(),
                     tuple(np.array(x).copy() for x in live)))
        st = G.decode_ex_game(live[0], P)
        v = st["velocities"].astype(np.float64)
        clamped += int((np.hypot(v[..., 0], v[..., 1]) >= 6.9999).sum())
        rot = st["rotations"].astype(np.float64)
        if prev_rot is not None:
            wrapped += int((np.abs(rot - prev_rot) > 3.0).sum())
        prev_rot = rot
    orc.close()
    # the pinned inputs did not go quiet: a rotation wrapped and a ship reached the speed limit
    assert wrapped >= 1, "no rotation wrapped"
    assert clamped >= 1, "no lane reached the speed clamp"
    _oracle_runs[key] = (inputs, recs)
    return _oracle_runs[key]


def partition(kind, cd):
    n = total_ticks(cd) - (cd + 1)
    if kind == "one_launch":
        return [n]
    if kind == "one_tick_per_launch":
        return [1] * n
    head = [2, cd, cd + 1, cd + 2, 1]
    assert n - sum(head) >= 1
    return head + [n - sum(head)]


def compare(sess, rec, where):
    frames, imgs, cs, (oimg, odcs, ofr) = rec
    seen = 0
    for w, fr in enumerate(frames):
        if fr < 0:
            continue
        gimg, gcs = sess.read_cell(int(fr))
        np.testing.assert_array_equal(gimg, imgs[w], err_msg=f"{where}: cell image frame {fr}")
        np.testing.assert_array_equal(gcs, cs[w], err_msg=f"{where}: cell checksum frame {fr}")
        seen += 1
    assert seen >= 1
    gimg, gdcs, gfr = sess.read_live()
    np.testing.assert_array_equal(gimg, oimg, err_msg=f"{where}: live image")
    np.testing.assert_array_equal(gdcs, odcs, err_msg=f"{where}: display checksum")
    np.testing.assert_array_equal(gfr, ofr, err_msg=f"{where}: display frame")


@pytest.mark.parametrize("kind", ["one_launch", "one_tick_per_launch", "mixed"])
@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("P", PLAYERS)
def test_launch_partition_does_not_matter(gpu_available, P, cd, kind):
    import torch
    inputs, recs = oracle_run(P, cd)
    sess = (G.SessionBuilder(G.Game.EX_GAME, num_sessions=S).with_num_players(P).with_max_prediction_window(cd + 1)
            .with_check_distance(cd).with_input_delay(DELAY).start_synctest_session())
    dev = torch.from_numpy(inputs).cuda()
    t = cd + 1
    assert sess.run_ticks(dev[:t]) == t  # start-up: one launch per tick
    compare(sess, recs[t - 1], "after the start-up ticks")
    for n in partition(kind, cd):
        assert sess.run_ticks(dev[t:t + n]) == n
        t += n
        compare(sess, recs[t - 1], f"after the launch of {n} ticks ending at tick {t}")
        assert (sess.mismatches() == G.NULL_FRAME).all()
    assert t == inputs.shape[0]
    sess.close()
