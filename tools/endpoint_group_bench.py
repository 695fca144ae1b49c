"""What the grouped packet codec costs per call against the `_all` codec moving the same inputs as
one stream per handle, and this tree's one-tick call against the parent commit's, in one process.

Shapes: ex_game's 1-byte inputs, 65,536 sessions, P = 4, a ring of 128 frames, 32-byte packet rows,
one new frame per endpoint per call plus two re-sent frames (the sender is acked two frames late).
The calls of a round alternate on one stream, each between its own pair of device events, the
parent's library first and last in every round.  Every line calls the C entry points through ctypes
with the same arguments' worth of host work:

    a1, a2      rb_p2p_run_ticks of one tick from the parent commit's library (--parent-lib); two
                of them, so the run shows what the same code measures against itself
    b           the same call from this tree's library
    all-d/-e    rb_decode_input_packets_all / rb_encode_input_packets_all, handle mask 0b1111: four
                endpoints per session, four packets
    spec-d/-e   rb_decode_input_packets_grouped / rb_encode_input_packets_grouped, the spectator
                group {0,1,2,3}: one endpoint per session, one packet of 4-byte frames
    pair-d/-e   the same with the groups {0,1}{2,3}: two endpoints per session, 2-byte frames

The rule is tools/ab.py's: b differs from the parent only beyond three times the parent's own
median absolute deviation (a1 and a2 pooled).  The codec lines are reported as ratios against the
`_all` line of the same direction; nothing gates anything.

    python3 tools/endpoint_group_bench.py --parent-lib /path/to/parent/libggrs_amd.so
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
R, W, STRIDE, BACK, LEAD, P = 128, 8, 32, 2, 16, 4


def mad(v, m):
    return statistics.median(abs(x - m) for x in v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libggrs_amd.so built from the parent commit")
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=12, help="timed rounds (at least 12)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "endpoint_groups_ab.log"))
    args = ap.parse_args()
    if args.rounds < 12:
        raise SystemExit("at least 12 timed rounds")

    import torch

    import ggrs_amd as G
    from ggrs_amd import _lib as L
    from time_sync_bench import make_batch, open_lib

    if not torch.cuda.is_available():
        raise SystemExit("endpoint_group_bench needs a GPU: nothing is measured without one")
    S, delay = args.sessions, 2
    n = args.warmup + args.rounds
    T = n + LEAD + BACK + 2
    dev = torch.device("cuda", 0)
    here, parent = L.load(), open_lib(args.parent_lib)
    stream = torch.cuda.Stream(device=dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    z = lambda shape, dt, v=0: torch.full(shape, v, dtype=dt, device=dev)
    sets = {"all": None, "spec": G.EndpointGroups.spectator(P), "pair": G.EndpointGroups([[0, 1], [2, 3]], P)}
    names = ["a1", "b"] + [f"{k}-{d}" for d in "de" for k in sets] + ["a2"]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with torch.cuda.stream(stream):
        dx = torch.from_numpy(G.synth_inputs(S, P, T + delay)).to(dev)  # [T, P, S] by frame
        t = torch.arange(T, dtype=torch.int32, device=dev)
        upto_t = torch.clamp(t - 2, min=-1)[:, None, None].expand(T, P, S).contiguous()
        ring_truth = z((R, P, S), torch.uint8)
        ring_truth[torch.arange(T, device=dev) & (R - 1)] = dx[:T]
        ack = [z((P, S), torch.int32, i - 1) for i in range(n)]
        new = [z((P, S), torch.int32, i + BACK) for i in range(n)]

        def decode(k, i, ring, status):
            pk, ln, st = packets[k]
            if sets[k] is None:
                rc = here.rb_decode_input_packets_all(0, sp, 0b1111, P, S, 1, W, p(pk[i]), STRIDE, p(ln[i]), p(st[i]), p(ring.inputs), R,
                                                      R, p(ring.upto), p(status))
            else:
                rc = here.rb_decode_input_packets_grouped(0, sp, sets[k].packed, P, S, 1, W, p(pk[i]), STRIDE, p(ln[i]), p(st[i]),
                                                          p(ring.inputs), R, R, p(ring.upto), p(status))
            assert rc == 0

        def encode(k, i, o):
            if sets[k] is None:
                rc = here.rb_encode_input_packets_all(0, sp, 0b1111, P, S, 1, p(ring_truth), R, R, 0, p(ack[i]), p(new[i]), p(o[0]), STRIDE,
                                                      p(o[1]), p(o[2]))
            else:
                rc = here.rb_encode_input_packets_grouped(0, sp, sets[k].packed, P, S, 1, p(ring_truth), R, R, 0, p(ack[i]), p(new[i]),
                                                          p(o[0]), STRIDE, p(o[1]), p(o[2]))
            assert rc == 0

        # every round's packets (frames i .. i + BACK against frame i - 1), made once with this tree's encoders
        packets = {k: (z((n, P, S, STRIDE), torch.uint8), z((n, P, S), torch.int32), z((n, P, S), torch.int32)) for k in sets}
        for k in sets:
            for i in range(n):
                encode(k, i, tuple(x[i] for x in packets[k]))
            leads = list(range(P)) if sets[k] is None else list(sets[k].leads)
            assert int(packets[k][1][:, leads].min()) > 0
        rings = {k: G.DeliveryRing(R, P, S) for k in sets}
        status = {k: z((P, S), torch.int32) for k in sets}
        out = {k: (z((P, S, STRIDE), torch.uint8), z((P, S), torch.int32), z((P, S), torch.int32)) for k in sets}
        batch = {k: make_batch(parent if k in ("a1", "a2") else here, S, P, delay) for k in ("a1", "b", "a2")}
        for b in batch.values():
            b.set_stream(stream)
            b.run_ticks(dx[:LEAD], upto_t[:LEAD], dx)
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2 * len(names))] for _ in range(n)]
        for i in range(n):
            a = LEAD + i
            for j, name in enumerate(names):
                ev[i][2 * j].record(stream)
                if name in batch:
                    batch[name].run_ticks(dx[a:a + 1], upto_t[a:a + 1], dx)
                elif name.endswith("-d"):
                    decode(name[:-2], i, rings[name[:-2]], status[name[:-2]])
                else:
                    encode(name[:-2], i, out[name[:-2]])
                ev[i][2 * j + 1].record(stream)
        torch.cuda.synchronize()
        us = {name: [ev[i][2 * j].elapsed_time(ev[i][2 * j + 1]) * 1e3 for i in range(args.warmup, n)] for j, name in enumerate(names)}
        top = n - 1 + BACK
        g = torch.arange(top + 1, device=dev)
        for k in sets:  # every line decoded the same frames and encoded the schedule's packets
            assert (rings[k].upto == top).all() and torch.equal(rings[k].inputs[g & (R - 1)], dx[:top + 1]), k
            assert torch.equal(out[k][1], packets[k][1][n - 1]), k
        frames = [bt.frames()[0] for bt in batch.values()]
        assert all((f == frames[0]).all() for f in frames)
        for bt in batch.values():
            bt.close()

    med = {k: statistics.median(v) for k, v in us.items()}
    for k in names:
        say(f"{k:7s} median {med[k]:8.2f} us per call  MAD {mad(us[k], med[k]):5.2f}  min {min(us[k]):8.2f}  max {max(us[k]):8.2f}")
    base = us["a1"] + us["a2"]
    bm = statistics.median(base)
    bd = mad(base, bm)
    d = med["b"] - bm
    word = "slower" if d > 3 * bd else ("faster" if d < -3 * bd else "within the spread")
    say(f"tick: parent (a1, a2 pooled) median {bm:.2f} us, MAD {bd:.2f}, a1 against a2 {med['a1'] - med['a2']:+.2f} us")
    say(f"tick: b vs parent: {d:+.2f} us ({d / bm * 100:+.2f}%): {word} (3 MAD = {3 * bd:.2f} us)")
    results = {"tick_parent_us": round(bm, 2), "tick_parent_mad_us": round(bd, 2), "tick_here_us": round(med["b"], 2), "tick_verdict": word}
    for dname, d_ in (("decode", "d"), ("encode", "e")):
        for k in ("spec", "pair"):
            ratio = med[f"{k}-{d_}"] / med[f"all-{d_}"]
            say(f"{dname}: {k} / all = {ratio:.3f} ({med[f'{k}-{d_}']:.2f} us against {med[f'all-{d_}']:.2f} us)")
            results[f"{k}_{dname}_us"], results[f"{k}_{dname}_over_all"] = round(med[f"{k}-{d_}"], 2), round(ratio, 3)
        results[f"all_{dname}_us"] = round(med[f"all-{d_}"], 2)
    say(json.dumps({"bench": "endpoint_group_bench", "input_bytes": 1, "players": P, "sessions": S, "ring_frames": R,
                    "resent_frames": BACK, "timed_rounds": args.rounds, "warmup_rounds": args.warmup,
                    "device": torch.cuda.get_device_name(0), "results": results}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
