"""What per-session pacing costs a one-tick P2P call, against the parent commit's library, in one process.

Shape: ex_game, 2 players, 65,536 sessions, one tick per call, every delivery one tick late
(tools/time_sync_bench.py's network).  The batches run the same ticks on one stream, their calls
alternating, each between its own pair of device events; 3 warm-up calls, medians of 12:

    a1, a2  rb_p2p_run_ticks of the parent commit's library (--parent-lib: build the parent commit
            in a worktree and pass its ggrs_amd/libggrs_amd.so); two of them, so the run shows what
            the same code measures against itself
    b       this tree's rb_p2p_run_ticks
    c       rb_p2p_run_ticks_paced with a mask of all ones
    d       rb_p2p_run_ticks_paced with every 11th session parked, the parked set rotating per tick
    bt, ct, dt   b, c and d with time sync on (bt: the unpaced time-sync call)

    python3 tools/pacing_bench.py --parent-lib /path/to/parent/libggrs_amd.so
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libggrs_amd.so built from the parent commit")
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=12, help="timed calls of each batch (at least 12)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pacing_bench.json"))
    args = ap.parse_args()
    if args.calls < 12:
        raise SystemExit("at least 12 timed calls")

    import torch

    import ggrs_amd as G
    from ggrs_amd import _lib as L
    from time_sync_bench import make_batch, open_lib

    if not torch.cuda.is_available():
        raise SystemExit("pacing_bench needs a GPU: nothing is measured without one")
    S, P, delay = args.sessions, 2, 2
    T = args.warmup + args.calls
    dev = torch.device("cuda", 0)
    dx = torch.from_numpy(G.synth_inputs(S, P, T + delay)).to(dev)
    t = torch.arange(T, dtype=torch.int32, device=dev)
    upto = torch.clamp(t - 2, min=-1)[:, None, None].expand(T, P, S).contiguous()
    s = torch.arange(S, device=dev)
    ones = torch.ones((T, S), dtype=torch.uint8, device=dev)
    rot = ((s[None, :] + t[:, None]) % 11 != 0).to(torch.uint8).contiguous()  # every 11th session parked, rotating

    here, parent = L.load(), open_lib(args.parent_lib)
    names = ("a1", "b", "c", "d", "bt", "ct", "dt", "a2")
    mask_of = {"c": ones, "d": rot, "ct": ones, "dt": rot}
    batch = {n: make_batch(parent if n in ("a1", "a2") else here, S, P, delay) for n in names}
    stream = torch.cuda.Stream(device=dev)
    for b in batch.values():
        b.set_stream(stream)
    with torch.cuda.stream(stream):
        for n in ("bt", "ct", "dt"):
            batch[n].enable_time_sync(60)
            batch[n].receive_quality(1, torch.full((S,), 40, dtype=torch.int32, device=dev),
                                     torch.full((S,), 6, dtype=torch.int32, device=dev))
    us = {}
    with torch.cuda.stream(stream):
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)] for _ in range(T)]
        for i in range(T):
            ev[i][0].record(stream)
            for k, n in enumerate(names):
                m = mask_of.get(n)
                batch[n].run_ticks(dx[i:i + 1], upto[i:i + 1], dx, **({} if m is None else {"run_mask": m[i:i + 1]}))
                ev[i][k + 1].record(stream)
        torch.cuda.synchronize()
        for k, n in enumerate(names):
            us[n] = [ev[i][k].elapsed_time(ev[i][k + 1]) * 1e3 for i in range(args.warmup, T)]

    # every batch did its work: the unparked ones every tick, d and dt one tick in 11 less
    ref = batch["a1"]
    parked = (rot == 0).sum(0).cpu().numpy()
    for n in names:
        b = batch[n]
        assert (b.status()[0] == 0).all()
        if n in ("d", "dt"):
            assert (b.frames()[0] == T - parked).all() and (b.parked_ticks() == parked).all()
        else:
            assert (b.frames()[0] == T).all() and b.totals()[:3] == ref.totals()[:3]

    med = {n: statistics.median(us[n]) for n in names}
    a = 0.5 * (med["a1"] + med["a2"])
    res = {
        "bench": "pacing_bench", "game": "ex_game", "num_players": P, "sessions": S, "ticks_per_call": 1,
        "timed_calls": args.calls, "warmup_calls": args.warmup, "lag_frames": 1,
        "timing": "device events around each call, the batches' calls alternating on one stream",
        "configurations": {"a1": "parent commit, rb_p2p_run_ticks", "a2": "parent commit (again)",
                           "b": "this commit, rb_p2p_run_ticks", "c": "paced, mask of all ones",
                           "d": "paced, every 11th session parked (rotating)",
                           "bt": "this commit, rb_p2p_run_ticks, time sync on",
                           "ct": "paced, all ones, time sync on", "dt": "paced, every 11th parked, time sync on"},
        "device": torch.cuda.get_device_name(0),
    }
    res.update({f"{n}_us_per_call": round(med[n], 2) for n in names})
    res.update({f"{n}_min_max_us": [round(min(us[n]), 2), round(max(us[n]), 2)] for n in names})
    res["a_spread_us"] = round(abs(med["a1"] - med["a2"]), 2)  # the parent against itself
    res["b_minus_a_us"] = round(med["b"] - a, 2)
    res["c_minus_b_us"] = round(med["c"] - med["b"], 2)
    res["d_minus_b_us"] = round(med["d"] - med["b"], 2)
    res["ct_minus_bt_us"] = round(med["ct"] - med["bt"], 2)
    res["dt_minus_bt_us"] = round(med["dt"] - med["bt"], 2)
    res["us"] = {n: [round(v, 2) for v in us[n]] for n in names}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "us" and k != "configurations"}))
    for b in batch.values():
        b.close()


if __name__ == "__main__":
    main()
