"""What restarting sessions in place costs beside a one-tick P2P call, against the parent commit's library, in one process.

Shape: ex_game, 2 players, 65,536 sessions, one tick per call, every delivery one tick late
(tools/time_sync_bench.py's network).  The calls alternate on one stream, each between its own pair
of device events; 3 warm-up rounds, medians of 12:

    a1, a2  rb_p2p_run_ticks of the parent commit's library (--parent-lib: build the parent commit
            in a worktree and pass its ggrs_amd/libggrs_amd.so), first and last in each round: what
            the same code measures against itself
    b       this tree's rb_p2p_run_ticks
    r64     rb_p2p_restart_sessions of 1,024 sessions, one in 64, the set rotating per round
    r1      rb_p2p_restart_sessions of one session: the call's fixed cost
    rall    rb_p2p_restart_sessions(NULL): all 65,536
    r64b    r64 on a brawler batch of 4,096 sessions (64 sessions of 74 KB each)

In a second pass every timed call is queued behind a 50-tick launch of another batch, so the host
is ahead of the device and the event pair holds the call's device time alone (b_q, r64_q, rall_q,
r64b_q); the first pass's figures include whatever the device waited for the host's side of the
call (its wall time is given as *_host_us).

rall and r64b are also given as bytes written per second (the planes of restart.hpp, counted
below) and as a fraction of the store-only stream of profiles/r02_calib_write.json, whose byte
count profiles/r06_calib_fetch.json confirms (WRITE_SIZE ratio 1.0).

    python3 tools/restart_bench.py --parent-lib /path/to/parent/libggrs_amd.so
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

QS_FIELDS = 5 + 17 * 4  # p2p.hpp kQsFields
QUEUE_LEN = 128


def fresh_bytes(nw, lanes, cs_bytes, input_bytes, players, window=8):
    """Bytes of one session's columns in the planes a plain P2P batch has (p2p_engine.hip core_planes)."""
    state = nw * lanes * 4
    return state * (1 + window) + window * (cs_bytes + 4) + QUEUE_LEN * players * input_bytes + QS_FIELDS * 4 + 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libggrs_amd.so built from the parent commit")
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--brawler-sessions", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=12, help="timed rounds (at least 12)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restart_bench.json"))
    args = ap.parse_args()
    if args.calls < 12:
        raise SystemExit("at least 12 timed rounds")

    import numpy as np
    import torch

    import ggrs_amd as G
    from ggrs_amd import _lib as L
    from ggrs_amd.p2p import PlayerType
    from time_sync_bench import make_batch, open_lib

    if not torch.cuda.is_available():
        raise SystemExit("restart_bench needs a GPU: nothing is measured without one")
    S, SB, P, delay = args.sessions, args.brawler_sessions, 2, 2
    T = args.warmup + args.calls
    dev = torch.device("cuda", 0)
    R = max(2 * T, 50) + 4  # rows: both passes' ticks of b, and the 50-tick launches of the second pass
    dx = torch.from_numpy(G.synth_inputs(S, P, R + delay)).to(dev)
    t = torch.arange(R, dtype=torch.int32, device=dev)
    upto = torch.clamp(t - 2, min=-1)[:, None, None].expand(R, P, S).contiguous()

    here, parent = L.load(), open_lib(args.parent_lib)
    batch = {"a1": make_batch(parent, S, P, delay), "a2": make_batch(parent, S, P, delay),
             "b": make_batch(here, S, P, delay), "r": make_batch(here, S, P, delay)}
    bb = G.SessionBuilder(G.Game.BRAWLER, num_sessions=SB).with_num_players(P).with_input_delay(delay)
    bb.add_player(PlayerType.Local, 0).add_player(PlayerType.Remote, 1)
    batch["rb"] = bb.start_p2p_session()
    stream = torch.cuda.Stream(device=dev)
    for b in batch.values():
        b.set_stream(stream)
    masks = [(np.arange(S) % 64 == i % 64).astype(np.uint8) for i in range(T)]
    bmasks = [(np.arange(SB) % 64 == i % 64).astype(np.uint8) for i in range(T)]
    names = ("a1", "b", "r64", "r1", "rall", "r64b", "a2")
    queued = ("b", "r64", "r1", "rall", "r64b")
    one = [(np.arange(S) == 64 * i + 7).astype(np.uint8) for i in range(T)]
    us, host_us = {}, {n: [] for n in names}
    batch["busy"] = make_batch(here, S, P, delay)
    batch["busy"].set_stream(stream)

    def call(n, i):
        t0 = time.perf_counter()
        if n in ("a1", "b", "a2"):
            batch[n].run_ticks(dx[i:i + 1], upto[i:i + 1], dx)
        elif n == "r64":
            batch["r"].restart_sessions(masks[i])
        elif n == "r1":
            batch["r"].restart_sessions(one[i])
        elif n == "rall":
            batch["r"].restart_sessions(None)
        else:
            batch["rb"].restart_sessions(bmasks[i])
        return (time.perf_counter() - t0) * 1e6

    with torch.cuda.stream(stream):
        # the restarted batches have played: their columns are not what a restart writes
        batch["r"].run_ticks(dx[:4], upto[:4], dx)
        batch["rb"].run_ticks(dx[:4, :, :SB].contiguous(), upto[:4, :, :SB].contiguous(), dx[:, :, :SB].contiguous())
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)] for _ in range(T)]
        for i in range(T):
            ev[i][0].record(stream)
            for k, n in enumerate(names):
                h = call(n, i)
                if i >= args.warmup:
                    host_us[n].append(h)
                ev[i][k + 1].record(stream)
        torch.cuda.synchronize()
        for k, n in enumerate(names):
            us[n] = [ev[i][k].elapsed_time(ev[i][k + 1]) * 1e3 for i in range(args.warmup, T)]
        # the second pass: each call behind a 50-tick launch, so that it waits on the device, not the host
        qev = {n: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(T)] for n in queued}
        for i in range(T):
            for n in queued:
                batch["busy"].restart_sessions(None)  # the same 50 ticks from frame 0 every time
                batch["busy"].run_ticks(dx[:50], upto[:50], dx)
                qev[n][i][0].record(stream)
                call(n, T + i if n == "b" else i)
                qev[n][i][1].record(stream)
            torch.cuda.synchronize()
        for n in queued:
            us[n + "_q"] = [qev[n][i][0].elapsed_time(qev[n][i][1]) * 1e3 for i in range(args.warmup, T)]

    # every batch did its work: the ticked ones every tick, the restarted ones are at frame 0 again
    ref = batch["a1"]
    for n in ("a1", "a2"):
        assert (batch[n].status()[0] == 0).all() and (batch[n].frames()[0] == T).all()
        assert batch[n].totals()[:3] == ref.totals()[:3]
    assert (batch["b"].status()[0] == 0).all() and (batch["b"].frames()[0] == 2 * T).all()  # both passes
    assert (batch["r"].frames()[0] == 0).all() and (batch["r"].read_cells()[0] == -1).all()
    fb = batch["rb"].frames()[0]
    assert (fb[np.arange(SB) % 64 < min(T, 64)] == 0).all() and (fb[np.arange(SB) % 64 >= T] == 4).all()

    med = {n: statistics.median(v) for n, v in us.items()}
    a = 0.5 * (med["a1"] + med["a2"])
    store = json.load(open(os.path.join(ROOT, "profiles", "r02_calib_write.json")))["store_only_GBps"]
    ex_b, br_b = fresh_bytes(5, 2, 2, 1, P), fresh_bytes(32, 64, 2, 1, P)
    res = {
        "bench": "restart_bench", "game": "ex_game", "num_players": P, "sessions": S, "brawler_sessions": SB,
        "ticks_per_call": 1, "timed_calls": args.calls, "warmup_calls": args.warmup, "lag_frames": 1,
        "timing": "device events around each call, the calls alternating on one stream",
        "configurations": {"a1": "parent commit, rb_p2p_run_ticks", "a2": "parent commit (again)",
                           "b": "this commit, rb_p2p_run_ticks",
                           "r64": "rb_p2p_restart_sessions, one session in 64 (rotating)",
                           "r1": "rb_p2p_restart_sessions, one session",
                           "rall": "rb_p2p_restart_sessions(NULL)",
                           "r64b": "rb_p2p_restart_sessions on the brawler batch, one session in 64"},
        "device": torch.cuda.get_device_name(0),
    }
    res.update({f"{n}_us_per_call": round(med[n], 2) for n in us})
    res.update({f"{n}_min_max_us": [round(min(us[n]), 2), round(max(us[n]), 2)] for n in us})
    res.update({f"{n}_host_us": round(statistics.median(host_us[n]), 2) for n in names})
    res["r64_q_minus_r1_q_us"] = round(med["r64_q"] - med["r1_q"], 2)  # the 1,023 other sessions' scattered stores
    res["a_spread_us"] = round(abs(med["a1"] - med["a2"]), 2)  # the parent against itself
    res["b_minus_a_us"] = round(med["b"] - a, 2)
    res["r64_over_b"] = round(med["r64"] / med["b"], 3)
    res["bytes_per_session"] = {"ex_game": ex_b, "brawler": br_b}
    res["store_only_GBps"] = store
    for n, nbytes in (("r64", ex_b * (S // 64)), ("rall", ex_b * S), ("r64b", br_b * (SB // 64))):
        gbps = nbytes / (med[n + "_q"] * 1e-6) / 1e9  # from the device time
        res[f"{n}_bytes"] = nbytes
        res[f"{n}_GBps"] = round(gbps, 1)
        res[f"{n}_fraction_of_store_only"] = round(gbps / store, 4)
    res["us"] = {n: [round(v, 2) for v in us[n]] for n in us}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "us" and k != "configurations"}))
    for b in batch.values():
        b.close()


if __name__ == "__main__":
    main()
