"""What endpoint liveness costs a one-tick P2P call, against the parent commit's library, in one process.

Shapes: ex_game, 2 and 4 players (handle 0 local), 65,536 sessions, one tick per call, every delivery
one tick late (tools/time_sync_bench.py's network).  The batches of a group run the same ticks on one
stream, their calls alternating, each between its own pair of device events, with the parent commit's
library first and last in every round; 3 warm-up rounds, medians of 12:

    a1, a2  rb_p2p_run_ticks of the parent commit's library (--parent-lib: build the parent commit in
            a worktree and pass its ggrs_amd/libggrs_amd.so); two of them, so the run shows what the
            same code measures against itself
    b       this tree's rb_p2p_run_ticks, liveness off
    c       one rb_p2p_poll_liveness with every endpoint healthy, then b's call
    d       c with one endpoint in 100 timing out in that poll (NetworkInterrupted and Disconnected
            in one poll, a second apart: the disconnect write included), another hundredth every round
    x       b's call, then one rb_p2p_export_local_inputs of one new frame per session: the other
            one-launch, few-words-per-session call at this shape, to set c - b beside
    po, xo  c's poll and x's export alone between the events (their tick untimed beside them): the
            form in which DESIGN.md section 16 reports rb_p2p_export_local_inputs
    e       what a caller does without the timers: a host mask of the same sessions and
            rb_p2p_disconnect_player (a copy of the mask and a stream synchronisation), then b's call

e drains the stream and the calls launched right behind it would be timed with the host's launch
latency in them: it runs after a2, outside the judged part of the round, and PADS untimed calls of a
spare batch follow it before the next round's a1.  The rule is tools/ab.py's: b against the parent counts as a loss (or a gain) only beyond three times the parent's
own median absolute deviation (a1 and a2 pooled).  c - b, x - b and d against e are reported, not judged.

    python3 tools/liveness_bench.py --parent-lib /path/to/parent/libggrs_amd.so
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
TIMEOUT, NOTIFY, POLL_MS = 240, 80, 1000
PADS = 8  # untimed one-tick calls behind e: the host is ahead of the device again before a1
LEAD = 3  # untimed ticks first: a player disconnected at frame 0 has nothing to resimulate from


def mad(v, m):
    return statistics.median(abs(x - m) for x in v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libggrs_amd.so built from the parent commit")
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=12, help="timed rounds (at least 12)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "liveness_ab.log"))
    args = ap.parse_args()
    if args.rounds < 12:
        raise SystemExit("at least 12 timed rounds")

    import numpy as np
    import torch

    import ggrs_amd as G
    from ggrs_amd import _lib as L
    from time_sync_bench import make_batch, open_lib

    if not torch.cuda.is_available():
        raise SystemExit("liveness_bench needs a GPU: nothing is measured without one")
    S, delay = args.sessions, 2
    n = args.warmup + args.rounds
    if n > 100:
        raise SystemExit("at most 100 rounds: every round times out another hundredth of the endpoints")
    dev = torch.device("cuda", 0)
    here, parent = L.load(), open_lib(args.parent_lib)
    stream = torch.cuda.Stream(device=dev)
    names = ("a1", "b", "c", "d", "x", "po", "xo", "a2", "e")
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for P in (2, 4):
        group = f"p{P}-1-tick"
        T = n + LEAD
        dx = torch.from_numpy(G.synth_inputs(S, P, T + delay)).to(dev)
        t = torch.arange(T, dtype=torch.int32, device=dev)
        upto = torch.clamp(t - 2, min=-1)[:, None, None].expand(T, P, S).contiguous()
        s = np.arange(S)
        gone = [s % 100 == i for i in range(n)]  # round i's silent hundredth (its handle 1)
        healthy = torch.ones((P, S), dtype=torch.uint8, device=dev)
        rc = []  # d's received bytes: a peer is heard until the round it times out in
        for i in range(n):
            r = np.ones((P, S), np.uint8)
            r[1, s % 100 <= i] = 0
            rc.append(torch.from_numpy(r).to(dev))
        host_mask = [np.ascontiguousarray(g, dtype=np.uint8) for g in gone]
        with torch.cuda.stream(stream):
            batch = {k: make_batch(parent if k in ("a1", "a2") else here, S, P, delay) for k in names + ("pad",)}
            for b in batch.values():
                b.set_stream(stream)
            for k in ("c", "d", "po"):
                batch[k].enable_liveness(TIMEOUT, NOTIFY)
                batch[k].poll_liveness(0, healthy)  # every endpoint stamped before the first round
            for b in batch.values():
                b.run_ticks(dx[:LEAD], upto[:LEAD], dx)
            sent = {k: torch.full((P, S), -1, dtype=torch.int32, device=dev) for k in ("x", "xo")}
            out = torch.zeros((T + delay, P, S), dtype=torch.uint8, device=dev)
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2 * len(names))] for _ in range(n)]
            for i in range(n):
                now, a = POLL_MS * (i + 1), LEAD + i
                for j, k in enumerate(names):
                    b = batch[k]
                    if k == "xo":
                        b.run_ticks(dx[a:a + 1], upto[a:a + 1], dx)
                    ev[i][2 * j].record(stream)
                    if k in ("c", "po"):
                        b.poll_liveness(now, healthy)
                    elif k == "d":
                        b.poll_liveness(now, rc[i])
                    elif k == "e":
                        b.disconnect_player(1, host_mask[i])
                    if k not in ("po", "xo"):
                        b.run_ticks(dx[a:a + 1], upto[a:a + 1], dx)
                    if k in ("x", "xo"):
                        b.export_local_inputs(out, sent[k])
                    ev[i][2 * j + 1].record(stream)
                    if k == "po":
                        b.run_ticks(dx[a:a + 1], upto[a:a + 1], dx)
                for _ in range(PADS):
                    batch["pad"].run_ticks(dx[a:a + 1], upto[a:a + 1], dx)
            torch.cuda.synchronize()
            us = {k: [ev[i][2 * j].elapsed_time(ev[i][2 * j + 1]) * 1e3 for i in range(args.warmup, n)]
                  for j, k in enumerate(names)}
            # every batch did its work; d and e disconnected the same players and ran on alike
            ref = batch["a1"]
            for k in ("a2", "b", "c", "x", "po", "xo"):
                assert (batch[k].status()[0] == 0).all() and (batch[k].frames()[0] == n + LEAD).all(), k
                assert batch[k].totals()[:3] == ref.totals()[:3], k
            assert all((v[0] == n + LEAD - 1 + delay).all() for v in sent.values())
            d, e = batch["d"], batch["e"]
            assert (d.status()[0] == 0).all() and (e.status()[0] == 0).all()
            want = (s % 100 < n).astype(np.int32)
            assert (d.read_queues()[:, 1, 7] == want).all() and (e.read_queues()[:, 1, 7] == want).all()
            assert (d.read_live() == e.read_live()).all() and (d.frames()[0] == e.frames()[0]).all()
            cnt, kinds, handles, values = d.network_events()
            assert (cnt == 2 * want).all() and (kinds[want == 1, :2] == [L.RB_NET_INTERRUPTED, L.RB_NET_DISCONNECTED]).all()
            assert (batch["c"].network_events()[0] == 0).all()
            for b in batch.values():
                b.close()
        med = {k: statistics.median(v) for k, v in us.items()}
        base = us["a1"] + us["a2"]
        bm = statistics.median(base)
        bd = mad(base, bm)
        for k in names:
            say(f"{group:12s} {k:3s} median {med[k]:8.2f} us per call  MAD {mad(us[k], med[k]):5.2f}  "
                f"min {min(us[k]):8.2f}  max {max(us[k]):8.2f}")
        diff = med["b"] - bm
        word = "loss" if diff > 3 * bd else ("gain" if diff < -3 * bd else "within the spread")
        say(f"{group:12s} parent (a1, a2 pooled) median {bm:.2f} us, MAD {bd:.2f}, a1 against a2 {med['a1'] - med['a2']:+.2f} us")
        say(f"{group:12s} b vs parent: {diff:+.2f} us ({diff / bm * 100:+.2f}%): {word} (3 MAD = {3 * bd:.2f} us)")
        say(f"{group:12s} c - b (a poll, every endpoint healthy): {med['c'] - med['b']:+.2f} us; "
            f"x - b (rb_p2p_export_local_inputs): {med['x'] - med['b']:+.2f} us (reported, not judged)")
        say(f"{group:12s} po (the poll alone): {med['po']:.2f} us; xo (rb_p2p_export_local_inputs alone): {med['xo']:.2f} us "
            f"(reported, not judged)")
        say(f"{group:12s} d - b (a poll, 1 endpoint in 100 timing out): {med['d'] - med['b']:+.2f} us; "
            f"e - b (host mask + rb_p2p_disconnect_player): {med['e'] - med['b']:+.2f} us; d vs e: {med['d'] - med['e']:+.2f} us "
            f"(reported, not judged)")
        results.append({"group": group, "num_players": P, **{f"{k}_us": round(med[k], 2) for k in names},
                        "parent_us": round(bm, 2), "parent_mad_us": round(bd, 2), "b_minus_parent_us": round(diff, 2),
                        "verdict": word, "c_minus_b_us": round(med["c"] - med["b"], 2),
                        "x_minus_b_us": round(med["x"] - med["b"], 2), "d_minus_b_us": round(med["d"] - med["b"], 2),
                        "e_minus_b_us": round(med["e"] - med["b"], 2), "d_minus_e_us": round(med["d"] - med["e"], 2)})

    say(json.dumps({"bench": "liveness_bench", "game": "ex_game", "sessions": S, "ticks_per_call": 1,
                    "timed_rounds": args.rounds, "warmup_rounds": args.warmup, "disconnect_timeout_ms": TIMEOUT,
                    "notify_start_ms": NOTIFY, "poll_interval_ms": POLL_MS, "device": torch.cuda.get_device_name(0),
                    "results": results}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if any(r["verdict"] == "loss" for r in results) else 0


if __name__ == "__main__":
    sys.exit(main())
