"""What exporting and importing sessions costs beside a one-tick P2P call and beside a restart of the same sessions,
against the parent commit's library, in one process (tools/restart_bench.py's method).

Shape: ex_game, 2 players, 65,536 sessions, one tick per call, every delivery one tick late.  The
calls alternate on one stream, each between its own pair of device events; 3 warm-up rounds,
medians of 12:

    a1, a2      rb_p2p_run_ticks of the parent commit's library (--parent-lib: build the parent commit
                in a worktree and pass its ggrs_amd/libggrs_amd.so), first and last in each round
    b           this tree's rb_p2p_run_ticks
    r64         the parent library's rb_p2p_restart_sessions of 1,024 sessions, one in 64, rotating
    e1, i1      rb_p2p_export_sessions / rb_p2p_import_sessions of one session: the calls' fixed cost
    e64, i64    of the same 1,024 sessions as r64, out of one batch and into another
    eall, iall  of all 65,536
    e64b, i64b  e64 and i64 on brawler batches of 4,096 sessions (64 records of 74 KB each)

In a second pass every timed call is queued behind a 50-tick launch of another batch, so the host
is ahead of the device and the event pair holds the call's device time alone (*_q); the first
pass's figures include whatever the device waited for the host's side of the call (its wall time
is given as *_host_us).

eall and iall are also given as bytes per second: record_bytes x S read and as many written, against
the store-only stream of profiles/r02_calib_write.json.

    python3 tools/migrate_bench.py --parent-lib /path/to/parent/libggrs_amd.so
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libggrs_amd.so built from the parent commit")
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--brawler-sessions", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=12, help="timed rounds (at least 12)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "migrate_bench.json"))
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
        raise SystemExit("migrate_bench needs a GPU: nothing is measured without one")
    S, SB, P, delay = args.sessions, args.brawler_sessions, 2, 2
    T = args.warmup + args.calls
    dev = torch.device("cuda", 0)
    R = max(2 * T, 50) + 4  # rows: both passes' ticks of b, and the 50-tick launches of the second pass
    dx = torch.from_numpy(G.synth_inputs(S, P, R + delay)).to(dev)
    t = torch.arange(R, dtype=torch.int32, device=dev)
    upto = torch.clamp(t - 2, min=-1)[:, None, None].expand(R, P, S).contiguous()

    def brawler():
        bb = G.SessionBuilder(G.Game.BRAWLER, num_sessions=SB).with_num_players(P).with_input_delay(delay)
        bb.add_player(PlayerType.Local, 0).add_player(PlayerType.Remote, 1)
        return bb.start_p2p_session()

    here, parent = L.load(), open_lib(args.parent_lib)
    batch = {"a1": make_batch(parent, S, P, delay), "a2": make_batch(parent, S, P, delay),
             "b": make_batch(here, S, P, delay), "r": make_batch(parent, S, P, delay),
             "src": make_batch(here, S, P, delay), "dst": make_batch(here, S, P, delay),
             "bsrc": brawler(), "bdst": brawler(), "busy": make_batch(here, S, P, delay)}
    stream = torch.cuda.Stream(device=dev)
    for b in batch.values():
        b.set_stream(stream)
    rb, rbb = batch["src"].record_bytes, batch["bsrc"].record_bytes
    assert rb == batch["dst"].record_bytes and rbb == batch["bdst"].record_bytes
    masks = [(np.arange(S) % 64 == i % 64).astype(np.uint8) for i in range(T)]
    lists = [np.nonzero(m)[0].astype(np.int32) for m in masks]          # r64's sessions
    blists = [np.nonzero(np.arange(SB) % 64 == i % 64)[0].astype(np.int32) for i in range(T)]
    one = [np.array([64 * i + 7], np.int32) for i in range(T)]
    everyone = np.arange(S, dtype=np.int32)
    names = ("a1", "b", "r64", "e1", "i1", "e64", "i64", "eall", "iall", "e64b", "i64b", "a2")
    queued = names[1:-1]
    us, host_us = {}, {n: [] for n in names}

    with torch.cuda.stream(stream):
        rec = {"1": torch.zeros((1, rb), dtype=torch.uint8, device=dev),
               "64": torch.zeros((len(lists[0]), rb), dtype=torch.uint8, device=dev),
               "all": torch.zeros((S, rb), dtype=torch.uint8, device=dev),
               "64b": torch.zeros((len(blists[0]), rbb), dtype=torch.uint8, device=dev)}

        def call(n, i):
            t0 = time.perf_counter()
            if n in ("a1", "b", "a2"):
                batch[n].run_ticks(dx[i:i + 1], upto[i:i + 1], dx)
            elif n == "r64":
                batch["r"].restart_sessions(masks[i % T])
            elif n == "e1":
                batch["src"].export_sessions(one[i % T], out=rec["1"])
            elif n == "i1":
                batch["dst"].import_sessions(one[i % T], rec["1"])
            elif n == "e64":
                batch["src"].export_sessions(lists[i % T], out=rec["64"])
            elif n == "i64":
                batch["dst"].import_sessions(lists[i % T], rec["64"])
            elif n == "eall":
                batch["src"].export_sessions(everyone, out=rec["all"])
            elif n == "iall":
                batch["dst"].import_sessions(everyone, rec["all"])
            elif n == "e64b":
                batch["bsrc"].export_sessions(blists[i % T], out=rec["64b"])
            else:
                batch["bdst"].import_sessions(blists[i % T], rec["64b"])
            return (time.perf_counter() - t0) * 1e6

        # the batches have played, the sources further than the destinations: no column holds what a
        # create wrote, and an import changes every plane
        bx, bu = dx[:, :, :SB].contiguous(), upto[:, :, :SB].contiguous()
        for n, k in (("r", 4), ("src", 6), ("dst", 3)):
            batch[n].run_ticks(dx[:k], upto[:k], dx)
        batch["bsrc"].run_ticks(bx[:6], bu[:6], bx)
        batch["bdst"].run_ticks(bx[:3], bu[:3], bx)
        # one call of each kind first: the lazily made groups and the staging slots exist before anything is timed
        for n in ("e1", "i1", "e64b", "i64b"):
            call(n, 0)
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
                call(n, T + i)
                qev[n][i][1].record(stream)
            torch.cuda.synchronize()
        for n in queued:
            us[n + "_q"] = [qev[n][i][0].elapsed_time(qev[n][i][1]) * 1e3 for i in range(args.warmup, T)]

    # every batch did its work: the destinations hold the sources' sessions, nothing was refused
    for n in ("a1", "a2"):
        assert (batch[n].status()[0] == 0).all() and (batch[n].frames()[0] == T).all()
    assert (batch["b"].status()[0] == 0).all() and (batch["b"].frames()[0] == 2 * T).all()  # both passes
    assert batch["dst"].import_refused() == 0 and batch["bdst"].import_refused() == 0
    assert (batch["dst"].frames()[0] == 6).all() and (batch["src"].frames()[0] == 6).all()
    assert np.array_equal(batch["dst"].read_live(), batch["src"].read_live())
    fb = batch["bdst"].frames()[0]
    assert (fb[np.arange(SB) % 64 < min(T, 64)] == 6).all() and (fb[np.arange(SB) % 64 >= T] == 3).all()

    med = {n: statistics.median(v) for n, v in us.items()}
    a = 0.5 * (med["a1"] + med["a2"])
    store = json.load(open(os.path.join(ROOT, "profiles", "r02_calib_write.json")))["store_only_GBps"]
    res = {
        "bench": "migrate_bench", "game": "ex_game", "num_players": P, "sessions": S, "brawler_sessions": SB,
        "ticks_per_call": 1, "timed_calls": args.calls, "warmup_calls": args.warmup, "lag_frames": 1,
        "timing": "device events around each call, the calls alternating on one stream",
        "configurations": {"a1": "parent commit, rb_p2p_run_ticks", "a2": "parent commit (again)",
                           "b": "this commit, rb_p2p_run_ticks",
                           "r64": "parent commit, rb_p2p_restart_sessions, one session in 64 (rotating)",
                           "e1": "rb_p2p_export_sessions, one session", "i1": "rb_p2p_import_sessions, one session",
                           "e64": "rb_p2p_export_sessions, r64's sessions", "i64": "rb_p2p_import_sessions, r64's sessions",
                           "eall": "rb_p2p_export_sessions, all sessions", "iall": "rb_p2p_import_sessions, all sessions",
                           "e64b": "e64 on the brawler batch", "i64b": "i64 on the brawler batch"},
        "device": torch.cuda.get_device_name(0),
        "record_bytes": {"ex_game": rb, "brawler": rbb},
    }
    res.update({f"{n}_us_per_call": round(med[n], 2) for n in us})
    res.update({f"{n}_min_max_us": [round(min(us[n]), 2), round(max(us[n]), 2)] for n in us})
    res.update({f"{n}_host_us": round(statistics.median(host_us[n]), 2) for n in names})
    res["a_spread_us"] = round(abs(med["a1"] - med["a2"]), 2)  # the parent against itself
    res["b_minus_a_us"] = round(med["b"] - a, 2)
    for n in ("e64", "i64"):
        res[f"{n}_over_r64"] = round(med[n] / med["r64"], 3)
        res[f"{n}_q_over_r64_q"] = round(med[n + "_q"] / med["r64_q"], 3)  # device time against device time
    res["e64_q_minus_e1_q_us"] = round(med["e64_q"] - med["e1_q"], 2)  # the 1,023 other sessions
    res["i64_q_minus_i1_q_us"] = round(med["i64_q"] - med["i1_q"], 2)
    res["store_only_GBps"] = store
    for n, nbytes in (("e64", rb * len(lists[0])), ("i64", rb * len(lists[0])), ("eall", rb * S), ("iall", rb * S),
                      ("e64b", rbb * len(blists[0])), ("i64b", rbb * len(blists[0]))):
        gbps = nbytes / (med[n + "_q"] * 1e-6) / 1e9  # from the device time; as many bytes read as written
        res[f"{n}_bytes_each_way"] = nbytes
        res[f"{n}_GBps_each_way"] = round(gbps, 1)
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
