"""The instruction-level forms of the fused ex_game SyncTest tick (games.hpp ExGame::prepare /
advance_prepared, device_math.hpp sincosf_glibc): the one-instruction position clamp, the wave-wide
choice of the speed clamp's division, the bit-operation selects of thrust, sine/cosine and
rotation.  Every one of them must leave each stored bit what the reference computes.

1. the position clamp as one median of three against the two-step form, every f32 bit pattern;
2. special values (signed zeros, denormals, infinities, NaNs, the clamp thresholds, the range
   limits of the rotation) injected into the cell a tick loads, through one-tick and fused launches;
3. parity with the oracle over partial waves and every lane-group size, long enough that speed
   clamps and rotation wraps occur.
"""
import ctypes

import numpy as np
import pytest

import ggrs_amd as G
from ggrs_amd.synth import synth_inputs
from oracle import oracle as O

pytestmark = pytest.mark.gpu

WIDTH, HEIGHT = np.float32(600.0), np.float32(800.0)


def f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def bits_of(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def neighbours(x):
    b = bits_of(x)
    return [f32(b - 1), np.float32(x), f32(b + 1)]


# ---------------------------------------------------------------------------- 1. position clamp
def test_position_clamp_median_equals_two_steps_every_pattern(gpu_available):
    """rb_debug_exgame_position_clamp over all 2^32 patterns (signalling NaNs left out by the entry
    point: an f32 add cannot produce them): the median form and max-then-min agree in every bit,
    for both limits."""
    from ggrs_amd import _lib as L
    lib = L.load()
    chunk = 1 << 28
    diff = (ctypes.c_uint64 * 2)()
    total = 0
    for first in range(0, 1 << 32, chunk):
        assert lib.rb_debug_exgame_position_clamp(0, first, chunk, diff, None) == 0
        assert diff[0] == 0, (int(diff[0]), hex(int(diff[1])), f32(int(diff[1]) & 0xFFFFFFFF))
        total += chunk
    assert total == 1 << 32
    # past the end of the pattern space, and an empty range
    assert lib.rb_debug_exgame_position_clamp(0, 0xFFFFFFFF, 2, diff, None) != 0
    assert lib.rb_debug_exgame_position_clamp(0, 0, 0, diff, None) != 0


def test_position_clamp_edges_equal_host(gpu_available):
    """The same entry point's results for an edge list against numpy's fmin(fmax(x, 0), L) on the host."""
    import torch
    from ggrs_amd import _lib as L
    lib = L.load()
    edges = [np.float32(0.0), np.float32(-0.0), f32(1), f32(0x80000001), f32(0x007FFFFF), f32(0x807FFFFF),
             np.float32(1e-40), np.float32(-1e-40), np.float32(np.inf), np.float32(-np.inf), f32(0x7FC00000),
             f32(0xFFC00000), np.float32(-1.0), np.float32(3e38), np.float32(-3e38)]
    edges += neighbours(WIDTH) + neighbours(HEIGHT)
    out = torch.empty(2, dtype=torch.float32, device="cuda")
    diff = (ctypes.c_uint64 * 2)()
    for x in edges:
        assert lib.rb_debug_exgame_position_clamp(0, bits_of(x), 1, diff, ctypes.c_void_p(out.data_ptr())) == 0
        assert diff[0] == 0, x
        got = out.cpu().numpy()
        with np.errstate(all="ignore"):
            want = np.array([np.fmin(np.fmax(x, np.float32(0)), WIDTH), np.fmin(np.fmax(x, np.float32(0)), HEIGHT)], np.float32)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=f"x = {x!r} ({bits_of(x):#x})")


# ---------------------------------------------------------------------------- 2. special values
P2, W8, CD7, D2 = 2, 8, 7, 2
WARM = 16  # ticks before the injection (8 start-up ticks, then steady ones)
UP, DOWN, LEFT, RIGHT = 1, 2, 4, 8


def word_offset(k, P):
    """Byte offset of canonical word k (positions, velocities, rotations) in the bincode image."""
    if k < 2 * P:
        return 20 + 4 * k
    if k < 4 * P:
        return 28 + 8 * P + 4 * (k - 2 * P)
    return 36 + 16 * P + 4 * (k - 4 * P)


def special_cases():
    """(words, target value, constant input or None) per victim session; player 0's words:
    x 0, y 1, vx 4, vy 5, rotation 8."""
    qnan = f32(0x7FC00000)
    cases = []
    for v in [np.float32(-0.0), qnan, np.float32(np.inf)] + neighbours(WIDTH):
        cases.append(((0,), v, None))
    for v in [np.float32(-0.0), qnan, np.float32(np.inf)] + neighbours(HEIGHT):
        cases.append(((1,), v, None))
    for v in [np.float32(0.0), np.float32(-0.0), np.float32(1e-40), np.float32(1e-30), np.float32(1e19), np.float32(3e38),
              np.float32(np.inf), qnan]:
        cases.append(((4,), v, None))
    thr = np.float32(np.float32(7.0) / np.sqrt(np.float32(2.0)))  # |v|^2 around 49: both components
    for v in neighbours(thr):
        cases.append(((4, 5), v, None))
        cases.append(((4, 5), v, UP))  # ... and thrust on top of it
    cases.append(((4,), np.float32(7.5), UP))   # a clamp whose other component is whatever the run left
    cases.append(((5,), np.float32(-1e-40), UP))
    two_pi = np.float32(2.0 * np.float32(np.pi))  # (float)(2 pi), ex_game's rem_euclid modulus
    below65 = f32(0x40D00000 - 1)
    for v, ins in ((np.float32(-0.0), (None,)), (below65, (0, LEFT, RIGHT)), (np.float32(6.5), (0, LEFT, RIGHT)),
                   (two_pi, (0, UP, LEFT, RIGHT, LEFT | RIGHT)), (np.float32(119.9), (0, RIGHT)), (qnan, (None, LEFT))):
        for i in ins:
            cases.append(((8,), v, i))
    return cases


def run_special(launch):
    """16 warm ticks, the injection into the cell the next tick loads, then `launch` ticks in one
    run_ticks call.  Returns (mismatch frames, live images) of the victims after checking both, and
    every session's live state, against the oracle."""
    import torch
    cases = special_cases()
    S = 64
    assert len(cases) <= S
    T = WARM + launch
    inputs = synth_inputs(S, P2, T + 1, seed=31, mask=0x0F)  # (one more row: the oracle's reporting tick, below)
    for v, (_, _, const) in enumerate(cases):
        if const is not None:
            inputs[:, :, v] = const
    sess = (G.SessionBuilder(G.Game.EX_GAME, num_sessions=S).with_num_players(P2).with_max_prediction_window(W8)
            .with_check_distance(CD7).with_input_delay(D2).start_synctest_session())
    orc = O.OracleBatch(O.EX_GAME, P2, W8, CD7, D2, S)
    dev = torch.from_numpy(inputs).cuda()
    assert sess.run_ticks(dev[:WARM]) == WARM
    for t in range(WARM):
        for h in range(P2):
            orc.add_local_input(h, inputs[t, h])
        kinds, _ = orc.advance()
        assert (kinds == 0).all()
    f = sess.current_frame() - CD7  # the cell the next tick loads
    img, _ = sess.read_cell(f)
    for v, (words, target, _) in enumerate(cases):
        for k in words:
            o = word_offset(k, P2)
            cur = int(img[v, o:o + 4].copy().view(np.uint32)[0])
            mask = cur ^ bits_of(target)
            assert mask != 0, (v, k, target)
            sess.debug_corrupt_cell(v, f, k, mask)
            orc.corrupt_cell(v, f, k, mask)
    img2, _ = sess.read_cell(f)
    for v, (words, target, _) in enumerate(cases):
        for k in words:
            o = word_offset(k, P2)
            assert int(img2[v, o:o + 4].copy().view(np.uint32)[0]) == bits_of(target)
    with pytest.raises(G.MismatchedChecksum) as ei:
        sess.run_ticks(dev[WARM:T])
    want = None
    for t in range(WARM, T):
        for h in range(P2):
            orc.add_local_input(h, inputs[t, h])
        kinds, frames = orc.advance()
        assert ((kinds == 0) | (kinds == 3)).all(), orc.last_panic()
        if (kinds != 0).any():
            want = np.where(kinds == 3, frames, -1)
    gimg, gcs, gfr = sess.read_live()
    oimg, ocs, ofr = orc.read_live()
    bad = np.nonzero((gimg != oimg).any(axis=1))[0]
    assert bad.size == 0, [(int(v), cases[v] if v < len(cases) else None) for v in bad]
    np.testing.assert_array_equal(gcs, ocs)
    np.testing.assert_array_equal(gfr, ofr)
    if want is None:
        # The reference compares a tick's resimulated checksums at the start of the next
        # advance_frame; the batch reports them with the launch that computed them.  One more
        # oracle tick yields the frames the one-tick launch already reported.
        assert launch == 1
        for h in range(P2):
            orc.add_local_input(h, inputs[T, h])
        kinds, frames = orc.advance()
        assert ((kinds == 0) | (kinds == 3)).all(), orc.last_panic()
        want = np.where(kinds == 3, frames, -1)
    victims = np.arange(len(cases))
    print("mismatch frames (device):", ei.value.frames[victims].tolist())
    print("mismatch frames (oracle):", want[victims].tolist())
    np.testing.assert_array_equal(ei.value.frames, want)
    assert (want[victims] != -1).all() and (want[len(cases):] == -1).all()
    sess.close()
    return ei.value.frames[victims].copy(), gimg[victims].copy()


_special_results = {}


@pytest.mark.parametrize("launch", [1, 5, 24])
def test_special_values_through_the_tick_like_oracle(gpu_available, launch):
    """Parent build: every case of special_cases() already matched the oracle (none dropped)."""
    _special_results[launch] = run_special(launch)


def test_special_values_one_tick_path_equals_fused_path(gpu_available):
    """The victims freeze at the tick after the injection whatever the launch length: the one-tick
    launch and the fused launches leave the same mismatch frames and the same live state."""
    for launch in (1, 5, 24):
        if launch not in _special_results:
            _special_results[launch] = run_special(launch)
    f1, i1 = _special_results[1]
    for launch in (5, 24):
        fl, il = _special_results[launch]
        np.testing.assert_array_equal(fl, f1)
        np.testing.assert_array_equal(il, i1)


# ---------------------------------------------------------------------------- 3. lane groups
@pytest.mark.parametrize("cd", [1, 7])
@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_lane_groups_partial_wave_clamps_and_wraps(gpu_available, P, cd):
    import torch
    S, T, W, d = 70, 90, 8, 2
    inputs = synth_inputs(S, P, T, seed=300 + 10 * P + cd, mask=0x0F)
    # Sessions that thrust straight all the way reach the speed clamp after 42 ticks (v -> 0.98 v
    # + 0.25 passes 7), sessions that turn all the way wrap their rotation; some of each in the
    # first wave and in the partial last one.
    inputs[:, :, 0] = UP
    inputs[:, :, 1] = UP | LEFT
    inputs[:, :, 2] = RIGHT
    inputs[:, :, S - 1] = UP
    inputs[:, :, S - 2] = DOWN | LEFT
    inputs[:, :, S - 3] = DOWN | RIGHT
    sess = (G.SessionBuilder(G.Game.EX_GAME, num_sessions=S).with_num_players(P).with_max_prediction_window(W)
            .with_check_distance(cd).with_input_delay(d).start_synctest_session())
    orc = O.OracleBatch(O.EX_GAME, P, W, cd, d, S)
    dev = torch.from_numpy(inputs).cuda()
    frames, imgs, valid, cs = None, None, None, None
    clamped = wrapped = 0
    prev_rot = None
    t = 0
    while t < T:
        n = min(23, T - t)
        assert sess.run_ticks(dev[t:t + n]) == n
        for k in range(t, t + n):
            for h in range(P):
                orc.add_local_input(h, inputs[k, h])
            kinds, _ = orc.advance()
            assert (kinds == 0).all()
            st = G.decode_ex_game(orc.read_live()[0], P)
            v = st["velocities"].astype(np.float64)
            clamped += int((np.hypot(v[..., 0], v[..., 1]) >= 6.9999).sum())
            rot = st["rotations"].astype(np.float64)
            if prev_rot is not None:
                wrapped += int((np.abs(rot - prev_rot) > 3.0).sum())
            prev_rot = rot
        t += n
        frames, imgs, valid, cs = orc.read_cells()
        for w, fr in enumerate(frames):
            if fr < 0:
                continue
            gimg, gcs = sess.read_cell(int(fr))
            np.testing.assert_array_equal(gimg, imgs[w], err_msg=f"cell image frame {fr}")
            np.testing.assert_array_equal(gcs, cs[w], err_msg=f"cell checksum frame {fr}")
        gimg, gdcs, gfr = sess.read_live()
        oimg, odcs, ofr = orc.read_live()
        np.testing.assert_array_equal(gimg, oimg)
        np.testing.assert_array_equal(gdcs, odcs)
        np.testing.assert_array_equal(gfr, ofr)
    assert (sess.mismatches() == G.NULL_FRAME).all()
    assert clamped >= 1, "no lane reached the speed clamp"
    assert wrapped >= 1, "no rotation wrapped"
    sess.close()
