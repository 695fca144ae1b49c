"""What time sync costs a P2P batch, against the parent commit's library, in one process.

Shape: ex_game, 2 players, 65,536 sessions, every delivery one tick late (tools/spectator_bench.py's
network), launches of 50 ticks and of one tick.  Four batches run the same ticks on one stream,
their launches alternating, each between its own pair of device events:

    a1, a2  the parent commit's library (--parent-lib: build the parent commit in a worktree and
            pass its ggrs_amd/libggrs_amd.so); two of them, so the run shows what the same code
            measures against itself
    b       this tree's library, time sync off (the tick log pointer is null: the same kernels)
    c       this tree's library, time sync on: the P2P launch and p2p_time_sync_kernel together

    python3 tools/time_sync_bench.py --parent-lib /path/to/parent/libggrs_amd.so
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def open_lib(path):
    """A second copy of the engine (another build): the signatures of ggrs_amd._lib on the entry points it has."""
    from ggrs_amd import _lib as L
    lib = ctypes.CDLL(path)
    for name, res, args in L.SIGNATURES:
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
    return lib


def make_batch(lib, S, P, delay):
    """SessionBuilder.start_p2p_session over `lib`: handle 0 local, handle 1 remote."""
    from ggrs_amd import _lib as L
    from ggrs_amd.p2p import P2PSession
    from ggrs_amd.session import game_of
    pc = L.RbP2PConfig()
    lib.rb_p2p_config_init(ctypes.byref(pc))
    pc.game, pc.num_sessions, pc.num_players, pc.input_delay, pc.local_mask = L.RB_GAME_EX_GAME, S, P, delay, 1
    h = ctypes.c_void_p()
    if lib.rb_p2p_create(ctypes.byref(pc), ctypes.byref(h)) != L.RB_OK:
        raise SystemExit((lib.rb_p2p_last_error(None) or b"").decode())
    return P2PSession(lib, h, game_of(pc.game), pc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libggrs_amd.so built from the parent commit")
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=12, help="timed launches of each batch and launch size (at least 12)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_sync_bench.json"))
    args = ap.parse_args()
    if args.launches < 12:
        raise SystemExit("at least 12 timed launches")

    import torch

    import ggrs_amd as G
    from ggrs_amd import _lib as L

    if not torch.cuda.is_available():
        raise SystemExit("time_sync_bench needs a GPU: nothing is measured without one")
    S, P, delay = args.sessions, 2, 2
    n = args.warmup + args.launches
    sizes = (50, 1)
    T = n * sum(sizes)
    dev = torch.device("cuda", 0)
    dx = torch.from_numpy(G.synth_inputs(S, P, T + delay)).to(dev)
    t = torch.arange(T, dtype=torch.int32, device=dev)
    upto = torch.clamp(t - 2, min=-1)[:, None, None].expand(T, P, S).contiguous()

    here, parent = L.load(), open_lib(args.parent_lib)
    names = ("a1", "b", "c", "a2")
    batch = {"a1": make_batch(parent, S, P, delay), "a2": make_batch(parent, S, P, delay),
             "b": make_batch(here, S, P, delay), "c": make_batch(here, S, P, delay)}
    stream = torch.cuda.Stream(device=dev)
    for b in batch.values():
        b.set_stream(stream)
    batch["c"].enable_time_sync(60)
    with torch.cuda.stream(stream):  # a session that runs ahead: events every 61 frames
        batch["c"].receive_quality(1, torch.full((S,), 40, dtype=torch.int32, device=dev),
                                   torch.full((S,), 6, dtype=torch.int32, device=dev))
    us = {}
    tick = 0
    with torch.cuda.stream(stream):
        for size in sizes:
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)] for _ in range(n)]
            for i in range(n):
                a, z = tick, tick + size
                ev[i][0].record(stream)
                for k, name in enumerate(names):
                    batch[name].run_ticks(dx[a:z], upto[a:z], dx)
                    ev[i][k + 1].record(stream)
                tick = z
            torch.cuda.synchronize()
            for k, name in enumerate(names):
                us[name, size] = [ev[i][k].elapsed_time(ev[i][k + 1]) * 1e3 for i in range(args.warmup, n)]

    # every batch did the same work, and time sync did its own
    ref = batch["a1"]
    for name in names:
        b = batch[name]
        assert (b.status()[0] == 0).all() and (b.frames()[0] == T).all(), "the sessions must advance every tick"
        assert b.totals()[:3] == ref.totals()[:3] and b.totals()[2] > 0, "the same rollbacks in every batch"
    counts, _, skips = batch["c"].wait_recommendations()
    assert (counts >= (T - 40) // 61).all() and (skips[:, 0] >= 3).all(), counts[:4]  # one event per 61 frames
    assert (batch["c"].frames_ahead() >= 3).all()

    res = {
        "bench": "time_sync_bench", "game": "ex_game", "num_players": P, "sessions": S, "timed_launches": args.launches,
        "warmup_launches": args.warmup, "lag_frames": 1,
        "timing": "device events around each call, the four batches' calls alternating on one stream",
        "configurations": {"a1": "parent commit", "a2": "parent commit (again)", "b": "this commit, time sync off",
                           "c": "this commit, time sync on (P2P launch + p2p_time_sync_kernel)"},
        "device": torch.cuda.get_device_name(0),
    }
    for size in sizes:
        med = {name: statistics.median(us[name, size]) for name in names}
        a = 0.5 * (med["a1"] + med["a2"])
        r = {f"{name}_us_per_launch": round(med[name], 2) for name in names}
        r.update({f"{name}_min_max_us": [round(min(us[name, size]), 2), round(max(us[name, size]), 2)] for name in names})
        r["a_spread_us"] = round(abs(med["a1"] - med["a2"]), 2)       # the parent against itself
        r["b_minus_a_us"] = round(med["b"] - a, 2)                    # a null tick-log pointer
        r["c_minus_a_us_per_launch"] = round(med["c"] - a, 2)
        r["c_minus_a_us_per_tick"] = round((med["c"] - a) / size, 3)
        r["us"] = {name: [round(v, 2) for v in us[name, size]] for name in names}
        res[f"ticks_per_launch_{size}"] = r
    # bytes time sync adds per session and tick at P = 2 (one remote handle), every tick reaching send_input:
    # p2p_kernel writes 2 log words; p2p_time_sync_kernel reads them, marks one consumed, reads the
    # delivery watermark, reads and writes both window slots; per session and launch it loads 13 state
    # words and stores 9
    res["added_bytes_per_session_tick"] = 8 + 8 + 4 + 4 + 16
    res["added_state_bytes_per_session_launch"] = (13 + 9) * 4
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({f"{size}": {k: v for k, v in res[f"ticks_per_launch_{size}"].items() if k != "us"} for size in sizes}))
    for b in batch.values():
        b.close()


if __name__ == "__main__":
    main()
