"""What the packet codec costs per tick, per handle and for all endpoints in one launch, linear and
ring, against the parent commit's library, in one process.

Shapes: ex_game's 1-byte inputs, 65,536 sessions, P = 2 (one remote handle) and P = 4 (three), one
new frame per endpoint per tick plus two re-sent frames (the sender is acked two frames late).  The
lines of a group run the same packets on one stream, their calls alternating, each between its own
pair of device events, with the parent's library first and last in every round.  Every line calls
the C entry points through ctypes with the same arguments' worth of host work, so the lines differ
by the launches and the kernels, not by a Python wrapper:

    a1, a2  the existing per-handle call (rb_decode_input_packets / rb_encode_input_packets) into /
            out of a linear tensor, one launch per remote handle, from the parent commit's library
            (--parent-lib); two of them, so the run shows what the same code measures against itself
    lin     rb_decode_input_packets_all / rb_encode_input_packets_all, ring_frames = 0
    ring    the same call on a ring of 128 frames
    stage   what a ring caller did before: the per-handle call into a linear staging tensor, then
            DeliveryRing.scatter per handle (decode); a gather of the frames' slots into a linear
            staging tensor with torch, then the per-handle call (encode)

The rule is tools/ab.py's: a line differs from the parent only beyond three times the parent's own
median absolute deviation (a1 and a2 pooled).  Every line is reported; none gates anything.

    python3 tools/wire_ring_bench.py --parent-lib /path/to/parent/libggrs_amd.so
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
R, W, STRIDE, BACK = 128, 8, 32, 2


def mad(v, m):
    return statistics.median(abs(x - m) for x in v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libggrs_amd.so built from the parent commit")
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=12, help="timed rounds of every group (at least 12)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wire_ring_ab.log"))
    args = ap.parse_args()
    if args.rounds < 12:
        raise SystemExit("at least 12 timed rounds")

    import torch

    import ggrs_amd as G
    from ggrs_amd import _lib as L
    from time_sync_bench import open_lib

    if not torch.cuda.is_available():
        raise SystemExit("wire_ring_bench needs a GPU: nothing is measured without one")
    S, n = args.sessions, args.warmup + args.rounds
    T = n + BACK + 2
    dev = torch.device("cuda", 0)
    here, parent = L.load(), open_lib(args.parent_lib)
    stream = torch.cuda.Stream(device=dev)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    names = ("a1", "lin", "ring", "stage", "a2")
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def judge(group, us):
        med = {k: statistics.median(v) for k, v in us.items()}
        base = us["a1"] + us["a2"]
        bm = statistics.median(base)
        bd = mad(base, bm)
        for k in us:
            say(f"{group:12s} {k:5s} median {med[k]:8.2f} us per tick  MAD {mad(us[k], med[k]):5.2f}  min {min(us[k]):8.2f}  "
                f"max {max(us[k]):8.2f}")
        say(f"{group:12s} parent (a1, a2 pooled) median {bm:.2f} us, MAD {bd:.2f}, a1 against a2 {med['a1'] - med['a2']:+.2f} us")
        out = {"group": group, "parent_us": round(bm, 2), "parent_mad_us": round(bd, 2)}
        for k in ("lin", "ring", "stage"):
            d = med[k] - bm
            word = "slower" if d > 3 * bd else ("faster" if d < -3 * bd else "within the spread")
            say(f"{group:12s} {k} vs parent: {d:+.2f} us ({d / bm * 100:+.2f}%): {word} (3 MAD = {3 * bd:.2f} us)")
            out[f"{k}_us"], out[f"{k}_verdict"] = round(med[k], 2), word
        say(f"{group:12s} ring vs stage: {med['ring'] - med['stage']:+.2f} us ({(med['ring'] - med['stage']) / med['stage'] * 100:+.2f}%)")
        results.append(out)

    with torch.cuda.stream(stream):
        for P in (2, 4):
            mask = ((1 << P) - 1) & ~1
            remotes = [h for h in range(P) if (mask >> h) & 1]
            truth = torch.from_numpy(G.synth_inputs(S, P, T)).to(dev)                 # [T, P, S] by frame
            f = torch.arange(T, device=dev)
            ring_truth = torch.zeros((R, P, S), dtype=torch.uint8, device=dev)
            ring_truth[f & (R - 1)] = truth
            # every tick's packets, made once with this tree's encoder: frames t .. t + BACK against frame t - 1
            pk = torch.zeros((n, P, S, STRIDE), dtype=torch.uint8, device=dev)
            ln = torch.zeros((n, P, S), dtype=torch.int32, device=dev)
            st = torch.zeros((n, P, S), dtype=torch.int32, device=dev)
            ack = [torch.full((P, S), i - 1, dtype=torch.int32, device=dev) for i in range(n)]
            new = [torch.full((P, S), i + BACK, dtype=torch.int32, device=dev) for i in range(n)]
            for i in range(n):
                G.encode_packets(truth, mask, new[i], ack[i], 0, pk[i], ln[i], st[i])
            assert int(ln[:, remotes].min()) > 0
            # ---- decode
            lin_in = {k: torch.zeros((T, P, S), dtype=torch.uint8, device=dev) for k in ("a1", "a2", "lin", "stage")}
            rings = {k: G.DeliveryRing(R, P, S) for k in ("ring", "stage")}
            upto = {k: torch.full((P, S), -1, dtype=torch.int32, device=dev) for k in names}
            status = torch.zeros((P, S), dtype=torch.int32, device=dev)
            ahead = torch.arange(BACK + 1, device=dev)[:, None]
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2 * len(names))] for _ in range(n)]

            sp = ctypes.c_void_p(stream.cuda_stream)

            def per_handle_decode(lib, i, inputs, up):
                for h in remotes:
                    assert lib.rb_decode_input_packets(0, sp, h, P, S, 1, W, p(pk[i, h]), STRIDE, p(ln[i, h]), p(st[i, h]),
                                                       p(inputs), T, p(up), p(status[h])) == 0

            def all_decode(i, inputs, frames, ring_frames, up):  # the C entry point, as the per-handle lines call theirs
                assert here.rb_decode_input_packets_all(0, sp, mask, P, S, 1, W, p(pk[i]), STRIDE, p(ln[i]), p(st[i]), p(inputs),
                                                        frames, ring_frames, p(up), p(status)) == 0

            for i in range(n):
                for j, k in enumerate(names):
                    ev[i][2 * j].record(stream)
                    if k in ("a1", "a2"):
                        per_handle_decode(parent, i, lin_in[k], upto[k])
                    elif k == "lin":
                        all_decode(i, lin_in[k], T, 0, upto[k])
                    elif k == "ring":
                        all_decode(i, rings[k].inputs, R, R, rings[k].upto)
                    else:
                        before = upto[k].clone()
                        per_handle_decode(here, i, lin_in[k], upto[k])
                        for h in remotes:  # the new frames (one per tick after the first) from the staging tensor into their slots
                            first = before[h] + 1
                            rows = lin_in[k][:, h].gather(0, (first[None].long() + ahead).clamp(0, T - 1))
                            rings[k].scatter(h, first, upto[k][h] - before[h], rows)
                    ev[i][2 * j + 1].record(stream)
            torch.cuda.synchronize()
            us = {k: [ev[i][2 * j].elapsed_time(ev[i][2 * j + 1]) * 1e3 for i in range(args.warmup, n)] for j, k in enumerate(names)}
            top = n - 1 + BACK
            for k in ("a1", "a2", "lin", "stage"):  # every line decoded the same frames
                assert (upto[k][remotes] == top).all() and torch.equal(lin_in[k][:top + 1, remotes], truth[:top + 1, remotes]), k
            for k in ("ring", "stage"):
                g = torch.arange(top + 1, device=dev)
                assert (rings[k].upto[remotes] == top).all() and torch.equal(rings[k].inputs[g & (R - 1)][:, remotes], truth[:top + 1, remotes]), k
            judge(f"decode-p{P}", us)
            # ---- encode
            out = {k: (torch.zeros((P, S, STRIDE), dtype=torch.uint8, device=dev), torch.zeros((P, S), dtype=torch.int32, device=dev),
                       torch.zeros((P, S), dtype=torch.int32, device=dev)) for k in names}
            stage_in = torch.zeros((BACK + 2, P, S), dtype=torch.uint8, device=dev)
            zero = torch.full((P, S), 0, dtype=torch.int32, device=dev)
            last = torch.full((P, S), BACK + 1, dtype=torch.int32, device=dev)
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2 * len(names))] for _ in range(n)]

            def per_handle_encode(lib, inputs, frames, acked, newest, o):
                for h in remotes:
                    assert lib.rb_encode_input_packets(0, sp, h, P, S, 1, p(inputs), frames, 0, p(acked[h]), p(newest[h]),
                                                       p(o[0][h]), STRIDE, p(o[1][h]), p(o[2][h])) == 0

            def all_encode(inputs, frames, ring_frames, acked, newest, o):
                assert here.rb_encode_input_packets_all(0, sp, mask, P, S, 1, p(inputs), frames, ring_frames, 0, p(acked),
                                                        p(newest), p(o[0]), STRIDE, p(o[1]), p(o[2])) == 0

            for i in range(1, n):  # (from tick 1 on: every packet has a reference input)
                for j, k in enumerate(names):
                    ev[i][2 * j].record(stream)
                    if k in ("a1", "a2"):
                        per_handle_encode(parent, truth, T, ack[i], new[i], out[k])
                    elif k == "lin":
                        all_encode(truth, T, 0, ack[i], new[i], out[k])
                    elif k == "ring":
                        all_encode(ring_truth, R, R, ack[i], new[i], out[k])
                    else:  # frames ack .. newest out of their slots into a staging tensor that starts at the ack
                        g = torch.arange(i - 1, i + BACK + 1, device=dev)
                        stage_in.copy_(ring_truth[g & (R - 1)])
                        per_handle_encode(here, stage_in, BACK + 2, zero, last, out[k])
                    ev[i][2 * j + 1].record(stream)
            torch.cuda.synchronize()
            us = {k: [ev[i][2 * j].elapsed_time(ev[i][2 * j + 1]) * 1e3 for i in range(max(args.warmup, 1), n)]
                  for j, k in enumerate(names)}
            for k in names:  # the last tick's packets are the schedule's
                assert torch.equal(out[k][1][remotes], ln[n - 1][remotes]), k
                live = torch.arange(STRIDE, device=dev)[None, None, :] < ln[n - 1][remotes][:, :, None]
                assert torch.equal(out[k][0][remotes][live], pk[n - 1][remotes][live]), k
            judge(f"encode-p{P}", us)

    say(json.dumps({"bench": "wire_ring_bench", "input_bytes": 1, "sessions": S, "ring_frames": R, "resent_frames": BACK,
                    "timed_rounds": args.rounds, "warmup_rounds": args.warmup, "device": torch.cuda.get_device_name(0),
                    "results": results}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
