"""ex_game (and the brawler's fan-out) over every input byte.

The reference's `Input { inp: u8 }` is Pod: any byte is a legal input.  State::advance reads
bits 0-3 only, while the InputQueue compares, predicts and ships the whole byte — so a byte
whose high nibble changes mispredicts and rolls back without changing the game, and the
device's decoders of the low nibble (games.hpp Dec, the window carry) and the fan-out's class
machinery (p2p.hpp InputCanon, AlphabetClasses, select_per_player, try_select, cand_find with
its 0xFF "unused slot" marker) must be right for bytes they were never fed.  Three streams:

  full    synth_network(..., mask=0xFF): 15 of 16 inputs are >= 16
  noise   the 0x0F stream with a fresh random high nibble every frame, locals and remotes:
          every confirmation mispredicts on the raw byte while the input class is unchanged
  held    remote players hold 0xFF, 0x00, 0xFF, 0x00, 0xF0, 0x00, ... in blocks of 4-40 frames
  high    the 0x0F hold stream with every high nibble set: no input is below 0xF0 (fan-out only)

Every comparison is bit-exact equality with the oracle (OracleBatch, OracleP2P); a fan-out
batch is additionally compared with its plain twin.
"""
import functools

import numpy as np
import pytest

import ggrs_amd as G
from ggrs_amd.p2p import PlayerType, synth_network
from oracle import oracle as O
from test_p2p import compare_state, drive_oracle, gpu_pair
from test_p2p_long_match import plan_calls

S, T = 200, 90  # three full waves and a ragged one; 90 ticks: one-tick, 7-tick and 29-tick launches all occur
SEED = 0x1D0


@functools.lru_cache(maxsize=None)
def network(kind, P, mask, rd, lag, S_=S, T_=T):
    """(local inputs [T, P, S], remote_upto [T, P, S], remote inputs by frame) of one stream; 'base'
    is the noise stream with its high nibbles cleared.  Computed once per shape and only read."""
    lo, hi = lag
    inputs, upto, rin = synth_network(S_, P, T_, mask, rd, lo, hi, mask=0xFF if kind in ("full", "held") else 0x0F)
    rng = np.random.default_rng(SEED + 16 * P + mask)
    if kind == "noise":
        inputs = inputs | (rng.integers(0, 16, inputs.shape, dtype=np.uint8) << 4).astype(np.uint8)
    elif kind == "high":
        inputs = inputs | np.uint8(0xF0)
    elif kind == "held":
        inputs = inputs.copy()
        for h in range(P):
            if (mask >> h) & 1:
                continue
            for s in range(S_):
                t, k = 0, 0
                while t < T_:
                    n = int(rng.integers(4, 41))
                    inputs[t:t + n, h, s] = 0x00 if k % 2 else (0xF0 if k % 4 == 0 and k else 0xFF)
                    t, k = t + n, k + 1
    else:
        assert kind in ("full", "base")
    rin = np.zeros_like(rin)
    rin[rd:] = inputs
    for a in (inputs, upto, rin):
        a.setflags(write=False)
    return inputs, upto, rin


def test_streams_cover_the_byte_domain():
    inputs, _, _ = network("full", 2, 0b01, 2, (0, 6))
    assert (inputs >= 16).mean() > 0.9 and len(np.unique(inputs)) == 256
    noise, _, _ = network("noise", 2, 0b01, 2, (0, 6))
    base, _, _ = network("base", 2, 0b01, 2, (0, 6))
    np.testing.assert_array_equal(noise & 0x0F, base)
    assert ((noise[1:] >> 4) != (noise[:-1] >> 4)).mean() > 0.9  # the raw byte changes nearly every frame
    held, _, rin = network("held", 2, 0b01, 2, (0, 6))
    assert set(np.unique(held[:, 1])) == {0x00, 0xF0, 0xFF}
    for s in range(S):  # the first distinct inputs of the remote player: 0xFF, 0x00, 0xFF (then 0x00, 0xF0)
        v = held[:, 1, s]
        d = v[np.r_[True, v[1:] != v[:-1]]]
        assert d[:3].tolist() == [0xFF, 0x00, 0xFF] and (len(d) < 5 or d[4] == 0xF0)


P2P_CASES = [  # P, W, d, rd, local_mask, sparse, lag range
    (2, 8, 2, 2, 0b01, False, (0, 6)),
    (3, 7, 0, 2, 0b010, True, (0, 4)),
    (4, 8, 1, 1, 0b0001, False, (1, 5)),
]
P2P_IDS = [f"P{c[0]}-W{c[1]}-sp{int(c[5])}" for c in P2P_CASES]


@pytest.mark.parametrize("case", P2P_CASES, ids=P2P_IDS)
def test_oracle_rolls_back_on_the_raw_byte_and_plays_the_low_nibble(case):
    """The schedule does what it is for, on the oracle alone: the nibble noise causes strictly more
    LoadGameState requests than the same network with the high nibbles cleared, and both runs end
    in the same live state; the full-byte and held streams play without a panic."""
    P, W, d, rd, mask, sparse, lag = case
    loads, live = {}, {}
    for kind in ("noise", "base", "full", "held"):
        inputs, upto, rin = network(kind, P, mask, rd, lag)
        orc = O.OracleP2P(O.EX_GAME, P, W, d, mask, S, sparse_saving=sparse, remote_delay=rd)
        res = drive_oracle(orc, mask, inputs, upto, rin, T)
        assert all((r[0] != O.KIND_PANIC).all() for r in res), orc.last_panic()
        loads[kind] = int(sum((r[1] != G.NULL_FRAME).sum() for r in res))
        live[kind] = orc.read_live()[0].copy()
        orc.close()
    assert loads["noise"] > loads["base"] > 0, loads
    np.testing.assert_array_equal(live["noise"], live["base"])


# ---------------------------------------------------------------------------- 1. SyncTest
def sync_inputs(kind, P):
    inputs = G.synth_inputs(S, P, 60, seed=SEED + P, mask=0xFF if kind == "full" else 0x0F)
    if kind == "noise":
        rng = np.random.default_rng(SEED + P)
        inputs = inputs | (rng.integers(0, 16, inputs.shape, dtype=np.uint8) << 4).astype(np.uint8)
    return inputs


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["full", "noise"])
@pytest.mark.parametrize("cd", [2, 7])
@pytest.mark.parametrize("P", [2, 4])
def test_gpu_synctest_over_every_byte(gpu_available, P, cd, kind):
    """Start-up ticks, a 20-tick fused call (the window carry), five one-tick calls, another fused
    call and the rest: cells, checksums, live images and mismatch words equal OracleBatch's after
    every call."""
    import torch
    inputs = sync_inputs(kind, P)
    assert (inputs >= 16).mean() > 0.9
    sess = (G.SessionBuilder(G.Game.EX_GAME, num_sessions=S).with_num_players(P).with_max_prediction_window(8)
            .with_check_distance(cd).with_input_delay(2).start_synctest_session())
    orc = O.OracleBatch(O.EX_GAME, P, 8, cd, 2, S)
    dev = torch.from_numpy(inputs).cuda()
    calls = [cd + 1, 20, 1, 1, 1, 1, 1, 20]
    calls.append(inputs.shape[0] - sum(calls))
    t = 0
    for n in calls:
        assert sess.run_ticks(dev[t:t + n]) == n
        for k in range(t, t + n):
            for h in range(P):
                orc.add_local_input(h, inputs[k, h])
            kinds, frames = orc.advance()
            assert (kinds == 0).all(), orc.last_panic()
        t += n
        np.testing.assert_array_equal(sess.mismatches(), np.where(kinds == 3, frames, G.NULL_FRAME))
        ofr, oimg, _, ocs = orc.read_cells()
        seen = 0
        for w, fr in enumerate(ofr):
            if fr < 0:
                continue
            img, cs = sess.read_cell(int(fr))
            np.testing.assert_array_equal(img, oimg[w], err_msg=f"cell image of frame {fr} after tick {t - 1}")
            np.testing.assert_array_equal(cs, ocs[w], err_msg=f"cell checksum of frame {fr} after tick {t - 1}")
            seen += 1
        assert seen >= min(t, cd)
        for got, want in zip(sess.read_live(), orc.read_live()):
            np.testing.assert_array_equal(got, want, err_msg=f"live state after tick {t - 1}")
    assert t == inputs.shape[0]
    sess.close()
    orc.close()


# ---------------------------------------------------------------------------- 2. P2P, plain and sparse
def run_calls(sess, orc, mask, net, calls):
    """The calls on the device and the same ticks on the oracle: the last tick's status, LoadGameState
    frame and request counts, and cells, live state, frames and queues, after every call."""
    import torch
    inputs, upto, rin = net
    di, du, dr = (torch.from_numpy(a.copy()).cuda() for a in net)
    for t0, t1 in calls:
        sess.run_ticks(di[t0:t1], du[t0:t1], dr)
        ost, olf, ona, ons = drive_oracle(orc, mask, inputs, upto, rin, t1, t0=t0)[-1]
        st, lf, na, ns = sess.status()
        np.testing.assert_array_equal(st, ost, err_msg=f"status, tick {t1 - 1}")
        np.testing.assert_array_equal(lf, olf, err_msg=f"LoadGameState frame, tick {t1 - 1}")
        np.testing.assert_array_equal(na, ona, err_msg=f"AdvanceFrame count, tick {t1 - 1}")
        np.testing.assert_array_equal(ns, ons, err_msg=f"SaveGameState count, tick {t1 - 1}")
        compare_state(sess, orc, t1 - 1)
    assert calls[-1][1] == T and sess.counters()[2] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["live", "q", "cells", "cells-lockstep"])
@pytest.mark.parametrize("kind", ["full", "noise"])
@pytest.mark.parametrize("case", P2P_CASES, ids=P2P_IDS)
def test_gpu_p2p_over_every_byte(gpu_available, monkeypatch, case, kind, plan):
    import torch
    P, W, d, rd, mask, sparse, lag = case
    if plan.startswith("cells"):
        monkeypatch.setenv("RB_P2P_SYNC_TICKS", "1" if plan == "cells-lockstep" else "0")
    net = network(kind, P, mask, rd, lag)
    sess, orc = gpu_pair(G.Game.EX_GAME, S, P, W, d, rd, mask, sparse)
    run_calls(sess, orc, mask, net, plan_calls(plan, upto=T))
    assert sess.totals()[2] > 0
    if kind == "noise":  # the high nibbles roll back and change nothing
        base, _ = gpu_pair(G.Game.EX_GAME, S, P, W, d, rd, mask, sparse)
        base.run_ticks(*(torch.from_numpy(a.copy()).cuda() for a in network("base", P, mask, rd, lag)))
        assert sess.totals()[2] > base.totals()[2] > 0, (sess.totals(), base.totals())
        np.testing.assert_array_equal(sess.read_live(), base.read_live())
        base.close()
    sess.close()
    orc.close()


# ---------------------------------------------------------------------------- 3. the fan-out
FAN_FORMS = {  # P, W, d, rd, local_mask, lag, candidates, per_player, generic (RB_FANOUT_GENERIC=1)
    "per-player-P4": (4, 8, 1, 1, 0b0001, (1, 5), 16, True, False),
    "per-player-P2": (2, 8, 2, 2, 0b01, (0, 6), 16, True, False),
    "one-player-P4": (4, 8, 1, 1, 0b0001, (1, 5), 16, False, False),
    "K8-P4": (4, 8, 1, 1, 0b0001, (1, 5), 8, False, False),
    "generic-P4": (4, 8, 1, 1, 0b0001, (1, 5), 16, False, True),
}
FAN_CASES = [(f, tpl) for f in FAN_FORMS for tpl in (1, 24) if not (FAN_FORMS[f][8] and tpl > 1)]


def run_fan(spec, plain, orc, mask, net, tpl, head=None):
    """spec (fan-out) and plain (its twin without) through the same launches: after every launch the
    last tick's status and request counts of both equal the oracle's, cells, live states, frames and
    queues of spec equal the oracle's (`head`: of its first sessions) and the twin's."""
    import torch
    inputs, upto, rin = net
    di, du, dr = (torch.from_numpy(a.copy()).cuda() for a in net)
    n = inputs.shape[2] if head is None else head
    for t0 in range(0, T, tpl):
        t1 = min(T, t0 + tpl)
        spec.run_ticks(di[t0:t1], du[t0:t1], dr)
        plain.run_ticks(di[t0:t1], du[t0:t1], dr)
        res = drive_oracle(orc, mask, inputs[:, :, :n], upto[:, :, :n], rin[:, :, :n], t1, t0=t0)[-1]
        for name, b in (("fan-out", spec), ("plain", plain)):
            for what, got, want in zip(("status", "rollback frame", "AdvanceFrame count", "SaveGameState count"),
                                       b.status(), res):
                np.testing.assert_array_equal(got[:n], want, err_msg=f"{name}: {what}, tick {t1 - 1}")
        for what, x, y in zip(("status", "rollback frame", "AdvanceFrame count", "SaveGameState count"),
                              spec.status(), plain.status()):
            np.testing.assert_array_equal(x, y, err_msg=f"fan-out vs plain: {what}, tick {t1 - 1}")
        compare_state(spec if head is None else Head(spec, n), orc, t1 - 1)
        np.testing.assert_array_equal(spec.read_live(), plain.read_live(), err_msg=f"live state vs plain, tick {t1 - 1}")
        for x, y in zip(spec.read_cells(), plain.read_cells()):
            np.testing.assert_array_equal(x, y, err_msg=f"cells vs plain, tick {t1 - 1}")
        np.testing.assert_array_equal(spec.read_queues(), plain.read_queues(), err_msg=f"queues vs plain, tick {t1 - 1}")
    ts, tp = spec.totals(), plain.totals()
    print(f"fan-out totals (advances, saves, loads, selects, branch frames) {ts}, plain {tp}")
    assert ts[2] + ts[3] == tp[2], (ts, tp)  # every rollback is a load or a select
    assert spec.counters()[2] == 0 and spec.counters()[1] == 0 and plain.counters()[2] == 0
    return ts


class Head:
    """The first n sessions of a batch, as compare_state reads them."""

    def __init__(self, sess, n):
        self.sess, self.n = sess, n

    def read_cells(self):
        return tuple(a[:, :self.n] for a in self.sess.read_cells())

    def read_live(self):
        return self.sess.read_live()[:self.n]

    def frames(self):
        return tuple(a[:self.n] for a in self.sess.frames())

    def read_queues(self):
        return self.sess.read_queues()[:self.n]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["full", "noise", "held", "high"])
@pytest.mark.parametrize("form,tpl", FAN_CASES, ids=[f"{f}-tpl{t}" for f, t in FAN_CASES])
def test_gpu_fanout_over_every_byte(gpu_available, monkeypatch, form, tpl, kind):
    P, W, d, rd, mask, lag, K, per_player, generic = FAN_FORMS[form]
    monkeypatch.setenv("RB_FANOUT_GENERIC", "1" if generic else "0")
    net = network(kind, P, mask, rd, lag)
    spec, orc = gpu_pair(G.Game.EX_GAME, S, P, W, d, rd, mask, False, fanout=True, candidates=K, per_player=per_player)
    plain, _ = gpu_pair(G.Game.EX_GAME, S, P, W, d, rd, mask, False)
    ts = run_fan(spec, plain, orc, mask, net, tpl)
    if kind == "full":  # nearly every input is >= 16: these selects happened on such bytes
        assert ts[3] > 0 and ts[4] > 0, ts
    # No input is below 0xF0 while the inputs are held as in the 0x0F stream: the forms whose branches are
    # input classes must find the class of such a byte.  (The generic form presimulates the raw values
    # 0-15 and compares raw bytes: it legitimately never selects here.)
    if kind == "high" and not generic:
        assert ts[3] > 0 and ts[4] > 0, ts
    spec.close()
    plain.close()
    orc.close()


# ---------------------------------------------------------------------------- 4. 0xFF as an input and as the unused-slot marker
def start_brawler(S_, P, W, d, rd, mask, K):
    b = (G.SessionBuilder(G.Game.BRAWLER, num_sessions=S_).with_num_players(P).with_max_prediction_window(W)
         .with_input_delay(d).with_remote_input_delay(rd))
    if K:
        b = b.with_speculative_fanout(True, K, adaptive=False, per_player=False)  # RB_P2P_FLAG_FANOUT_ALWAYS
    for h in range(P):
        b.add_player(PlayerType.Local if (mask >> h) & 1 else PlayerType.Remote, h)
    return b.start_p2p_session()


@pytest.mark.gpu
@pytest.mark.parametrize("tpl", [1, 10])
@pytest.mark.parametrize("K", [16, 8])
def test_gpu_brawler_fanout_looks_up_0xff_in_a_short_candidate_list(gpu_available, K, tpl):
    """The brawler's candidates are the queue's move-to-front list, 0xFF marking its unused slots
    (p2p.hpp cand_find): the remote player's first distinct inputs are 0xFF, 0x00, 0xFF, so 0xFF is
    looked up while the list is one or two entries long.  The fan-out batch equals its plain twin in
    every session and the oracle in the first 24."""
    P, W, d, rd, mask, lag, n = 2, 8, 1, 0, 0b01, (1, 5), 24  # remote delay 0: frame 0 already holds 0xFF
    net = network("held", P, mask, rd, lag)
    spec = start_brawler(S, P, W, d, rd, mask, K)
    plain = start_brawler(S, P, W, d, rd, mask, 0)
    orc = O.OracleP2P(O.BRAWLER, P, W, d, mask, n, sparse_saving=False, remote_delay=rd)
    ts = run_fan(spec, plain, orc, mask, net, tpl, head=n)
    assert ts[3] > 0 and ts[4] > 0, ts  # held inputs: selects happen
    spec.close()
    plain.close()
    orc.close()


# ---------------------------------------------------------------------------- 5. spectators
@pytest.mark.gpu
def test_gpu_spectators_of_a_full_byte_host(gpu_available):
    """A host batch on the full-byte stream feeds a spectator batch through export_confirmed_inputs:
    the spectator's state after frame c is the cell of frame c + 1 of the host's configuration with
    nothing predicted (the oracle), as tests/test_spectator.py states it."""
    import torch
    from test_spectator import DELAY, REMOTE_DELAY, Feed, assert_state_is_truth, host_truth, start_host, start_spectators
    P, mask, T_ = 2, 0b01, 80
    inputs, upto, rin = synth_network(S, P, T_ + 8, mask, REMOTE_DELAY, 1, 5, mask=0xFF)
    assert (rin >= 16).mean() > 0.9
    host = start_host(G.Game.EX_GAME, P, mask, S)
    spec = start_spectators(G.Game.EX_GAME, P, S)
    di, du, dr = (torch.from_numpy(a).cuda() for a in (inputs, upto, rin))
    feed = Feed(host, T_ + DELAY + 4)
    seen = host_truth(G.Game.EX_GAME, P, mask, inputs, rin, T_ + 8)
    for t in range(T_):
        host.run_ticks(di[t:t + 1], du[t:t + 1], dr)
        host.export_confirmed_inputs(feed.inputs, feed.upto, feed.last, feed.disc)
        spec.receive_host_status(feed.last.clone(), feed.disc.clone())
        spec.run_ticks(feed.upto.clone()[None].contiguous(), feed.inputs)
        if t % 10 == 9 or t == T_ - 1:
            assert_state_is_truth(spec, seen, f"tick {t}")
    cur, recv = spec.frames()
    assert cur.min() > 60 and (recv >= cur).all()
    got = feed.inputs.cpu().numpy()
    u = int(feed.upto.min())
    np.testing.assert_array_equal(got[:u + 1, 1], rin[:u + 1, 1])  # the exported remote inputs are the raw bytes
    host.close()
    spec.close()
