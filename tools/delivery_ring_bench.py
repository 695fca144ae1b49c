"""What the delivery ring's frame mask costs, against the parent commit's library, in one process.

Shapes: the default P2P line's (ex_game, 2 players, 65,536 sessions, 50-tick launches) and one tick
per call, every delivery one tick late (tools/time_sync_bench.py's network); the spectator launch
of tools/spectator_bench.py (50 ticks per launch); rb_p2p_export_local_inputs of one new frame per
session.  The batches of a group run the same ticks on one stream, their calls alternating, each
between its own pair of device events, with the parent commit's library first and last in every
round:

    a1, a2  the parent commit's library (--parent-lib: build the parent commit in a worktree and
            pass its ggrs_amd/libggrs_amd.so); two of them, so the run shows what the same code
            measures against itself
    lin     this tree, linear by-frame tensors (the default)
    ring    this tree, rb_p2p_set_delivery_ring(128) / rb_spectator_set_delivery_ring(128): the
            frames of each call are copied into their slots before its first event

The rule is tools/ab.py's: `lin` against the parent counts as a loss (or a gain) only beyond three
times the parent's own median absolute deviation (a1 and a2 pooled).  `ring` against `lin` is
reported, not judged.

    python3 tools/delivery_ring_bench.py --parent-lib /path/to/parent/libggrs_amd.so
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
R = 128


def make_spectators(lib, S, P):
    """SessionBuilder.start_spectator_session over `lib` (the builder's defaults)."""
    from ggrs_amd import _lib as L
    from ggrs_amd.session import game_of
    from ggrs_amd.spectator import SpectatorSession
    sc = L.RbSpectatorConfig()
    lib.rb_spectator_config_init(ctypes.byref(sc))
    sc.game, sc.num_sessions, sc.num_players = L.RB_GAME_EX_GAME, S, P
    h = ctypes.c_void_p()
    if lib.rb_spectator_create(ctypes.byref(sc), ctypes.byref(h)) != L.RB_OK:
        raise SystemExit((lib.rb_spectator_last_error(None) or b"").decode())
    return SpectatorSession(lib, h, game_of(sc.game), sc)


def mad(v, m):
    return statistics.median(abs(x - m) for x in v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libggrs_amd.so built from the parent commit")
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--ticks-per-launch", type=int, default=50)
    ap.add_argument("--launches", type=int, default=12, help="timed rounds of every group (at least 12)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delivery_ring_ab.log"))
    args = ap.parse_args()
    if args.launches < 12:
        raise SystemExit("at least 12 timed rounds")

    import torch

    import ggrs_amd as G
    from ggrs_amd import _lib as L
    from time_sync_bench import make_batch, open_lib

    if not torch.cuda.is_available():
        raise SystemExit("delivery_ring_bench needs a GPU: nothing is measured without one")
    S, P, delay, tpl = args.sessions, 2, 2, args.ticks_per_launch
    n = args.warmup + args.launches
    T = n * tpl
    assert tpl + 8 <= R, "a call's frames must fit the ring"
    dev = torch.device("cuda", 0)
    dx = torch.from_numpy(G.synth_inputs(S, P, T + delay)).to(dev)
    t = torch.arange(T, dtype=torch.int32, device=dev)
    lagged = torch.clamp(t - 2, min=-1)   # lag 1: before tick t the newest frame delivered is t - 2
    p2p_upto = lagged[:, None, None].expand(T, P, S).contiguous()
    spec_upto = lagged[:, None].expand(T, S).contiguous()
    ring = torch.zeros((R, P, S), dtype=torch.uint8, device=dev)

    def fill(a, z):
        """Frames a - 8 .. z - 1 (what the calls over ticks [a, z) can read) into their slots."""
        f = torch.arange(max(a - 8, 0), z, device=dev)
        ring[f & (R - 1)] = dx[f]

    here, parent = L.load(), open_lib(args.parent_lib)
    names = ("a1", "lin", "ring", "a2")
    lib_of = lambda k: parent if k in ("a1", "a2") else here
    stream = torch.cuda.Stream(device=dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def judge(group, us, unit):
        med = {k: statistics.median(v) for k, v in us.items()}
        base = us["a1"] + us["a2"]
        bm = statistics.median(base)
        bd = mad(base, bm)
        for k in us:
            say(f"{group:16s} {k:5s} median {med[k]:9.2f} us per {unit}  MAD {mad(us[k], med[k]):6.2f}  "
                f"min {min(us[k]):9.2f}  max {max(us[k]):9.2f}")
        d = med["lin"] - bm
        word = "loss" if d > 3 * bd else ("gain" if d < -3 * bd else "within the spread")
        say(f"{group:16s} parent (a1, a2 pooled) median {bm:.2f} us, MAD {bd:.2f}, a1 against a2 {med['a1'] - med['a2']:+.2f} us")
        say(f"{group:16s} lin vs parent: {d:+.2f} us ({d / bm * 100:+.2f}%): {word} (3 MAD = {3 * bd:.2f} us)")
        say(f"{group:16s} ring vs lin: {med['ring'] - med['lin']:+.2f} us ({(med['ring'] - med['lin']) / med['lin'] * 100:+.2f}%) (reported, not judged)")
        return {"group": group, "unit": unit, **{f"{k}_us": round(med[k], 2) for k in us}, "parent_us": round(bm, 2),
                "parent_mad_us": round(bd, 2), "lin_minus_parent_us": round(d, 2), "verdict": word,
                "ring_minus_lin_us": round(med["ring"] - med["lin"], 2)}

    results = []
    with torch.cuda.stream(stream):
        # ---- P2P ticks: tpl ticks per launch, then one tick per call
        for group, step, unit in ((f"p2p-{tpl}-ticks", tpl, "launch"), ("p2p-1-tick", 1, "call")):
            batch = {k: make_batch(lib_of(k), S, P, delay) for k in names}
            for b in batch.values():
                b.set_stream(stream)
            batch["ring"].set_delivery_ring(R)
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2 * len(names))] for _ in range(n)]
            for i in range(n):
                a, z = i * step, (i + 1) * step
                fill(a, z)
                for j, k in enumerate(names):
                    ev[i][2 * j].record(stream)
                    batch[k].run_ticks(dx[a:z], p2p_upto[a:z], ring if k == "ring" else dx)
                    ev[i][2 * j + 1].record(stream)
            torch.cuda.synchronize()
            us = {k: [ev[i][2 * j].elapsed_time(ev[i][2 * j + 1]) * 1e3 for i in range(args.warmup, n)]
                  for j, k in enumerate(names)}
            ref = batch["a1"]
            for k, b in batch.items():  # every batch did the same work
                assert (b.status()[0] == 0).all() and (b.frames()[0] == n * step).all(), k
                assert b.totals()[:3] == ref.totals()[:3] and b.totals()[2] > 0, k
            results.append(judge(group, us, unit))
            if step == 1:
                # ---- rb_p2p_export_local_inputs: one new frame per session after every one-tick call
                sent = {k: torch.full((P, S), -1, dtype=torch.int32, device=dev) for k in ("lin", "ring")}
                outs = {"lin": torch.zeros((T + delay, P, S), dtype=torch.uint8, device=dev), "ring": torch.zeros_like(ring)}
                for k in sent:
                    batch[k].export_local_inputs(outs[k], sent[k])   # everything so far: the next calls export one frame
                ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(n)]
                for i in range(n):
                    a = (n + i) * step
                    fill(a, a + 1)
                    for j, k in enumerate(("lin", "ring")):
                        batch[k].run_ticks(dx[a:a + 1], p2p_upto[a:a + 1], ring if k == "ring" else dx)
                        ev[i][2 * j].record(stream)
                        batch[k].export_local_inputs(outs[k], sent[k])
                        ev[i][2 * j + 1].record(stream)
                torch.cuda.synchronize()
                for j, k in enumerate(("lin", "ring")):
                    v = [ev[i][2 * j].elapsed_time(ev[i][2 * j + 1]) * 1e3 for i in range(args.warmup, n)]
                    assert (sent[k][0] == 2 * n - 1 + delay).all()
                    say(f"{'export-local':16s} {k:5s} median {statistics.median(v):9.2f} us per call (one new frame per session)  "
                        f"min {min(v):9.2f}  max {max(v):9.2f}")
                    results.append({"group": "export-local", "layout": k, "us": round(statistics.median(v), 2)})
                f = torch.arange(2 * n + delay, device=dev)
                assert torch.equal(outs["lin"][:2 * n + delay, 0], outs["ring"][f & (R - 1), 0])
            for b in batch.values():
                b.close()
        # ---- the spectator launch
        spec = {k: make_spectators(lib_of(k), S, P) for k in names}
        for b in spec.values():
            b.set_stream(stream)
        spec["ring"].set_delivery_ring(R)
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2 * len(names))] for _ in range(n)]
        for i in range(n):
            a, z = i * tpl, (i + 1) * tpl
            fill(a, z)
            for j, k in enumerate(names):
                ev[i][2 * j].record(stream)
                spec[k].run_ticks(spec_upto[a:z], ring if k == "ring" else dx)
                ev[i][2 * j + 1].record(stream)
        torch.cuda.synchronize()
        us = {k: [ev[i][2 * j].elapsed_time(ev[i][2 * j + 1]) * 1e3 for i in range(args.warmup, n)] for j, k in enumerate(names)}
        ref = spec["a1"]
        for k, b in spec.items():
            assert (b.frames()[0] == T - 3).all() and b.totals() == ref.totals(), k
            assert (b.read_live()[0] == ref.read_live()[0]).all(), k
        results.append(judge(f"spectator-{tpl}-ticks", us, "launch"))
        for b in spec.values():
            b.close()

    say(json.dumps({"bench": "delivery_ring_bench", "game": "ex_game", "num_players": P, "sessions": S, "ring_frames": R,
                    "timed_rounds": args.launches, "warmup_rounds": args.warmup, "device": torch.cuda.get_device_name(0),
                    "results": results}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if any(r.get("verdict") == "loss" for r in results) else 0


if __name__ == "__main__":
    sys.exit(main())
