"""What parsing and building GGRS's datagrams costs, against the parent commit's library, in one process.

Shapes: ex_game, 2 and 4 players (handle 0 local), 65,536 sessions.  The lines of a group run on one
stream, their calls alternating, each between its own pair of device events, with the parent commit's
library first and last in every round; 3 warm-up rounds, medians of 12.  Every line calls the C entry
points through ctypes:

    a1, a2  one-tick rb_p2p_run_ticks of the parent commit's library (--parent-lib); two of them, so
            the run shows what the same code measures against itself
    b       this tree's one-tick rb_p2p_run_ticks (the tick kernels are untouched: within the band)
    c       one rb_parse_datagrams_all, two slots, one Input (three frames) and one QualityReport per
            remote endpoint
    d       rb_decode_input_packets_all of the same Inputs' packets into a ring: the nearest existing
            one-launch, one-lane-per-endpoint call
    cb      one rb_build_datagrams_all writing those two datagrams per endpoint
    db      rb_encode_input_packets_all writing the same packets out of a ring
    e       c's parse as a caller does it today: the datagrams copied to the host, parsed with numpy
            into pinned tensors, the tensors copied back (it synchronises, so it runs after a2, outside
            the judged part of the round, and PADS untimed calls follow it)

The rule is tools/ab.py's: b against the parent counts as a loss (or a gain) only beyond three times
the parent's own median absolute deviation (a1 and a2 pooled).  c - d, cb - db and e / c are reported,
not judged.

    python3 tools/datagram_bench.py --parent-lib /path/to/parent/libggrs_amd.so
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
R, W, STRIDE, PSTRIDE, BACK, M = 128, 8, 64, 32, 2, 2
PADS, LEAD = 8, 3
NOW = 1_700_000_000_000


def mad(v, m):
    return statistics.median(abs(x - m) for x in v)


def host_parse(np, dg, ln, P, magic, out):
    """c's parse with numpy for the two kinds the run sends (slot 0 an Input, slot 1 a QualityReport),
    every check of the wire format included, into the pinned arrays of `out`."""
    off = 31 + 5 * P
    d0, d1 = dg[0].reshape(-1, STRIDE), dg[1].reshape(-1, STRIDE)
    n0, n1 = ln[0].reshape(-1), ln[1].reshape(-1)
    u32 = lambda d, at: d[:, at:at + 4].copy().view(np.uint32)[:, 0]
    u64 = lambda d, at: d[:, at:at + 8].copy().view(np.uint64)[:, 0]
    u16 = lambda d: d[:, 0:2].copy().view(np.uint16)[:, 0]
    plen = u64(d0, off - 8)
    ok0 = (n0 >= off) & (u16(d0) == magic) & (u32(d0, 2) == 2) & (u64(d0, 6) == P) & (d0[:, 14 + 5 * P] <= 1)
    for i in range(P):
        ok0 &= d0[:, 14 + 5 * i] <= 1
    ok0 &= plen <= (np.minimum(n0, STRIDE) - off).clip(0).astype(np.uint64)
    ok1 = (n1 >= 23) & (u16(d1) == magic) & (u32(d1, 2) == 4)
    out["received"][:] = (ok0 | ok1).reshape(out["received"].shape)
    ack = u32(d0, off - 12).view(np.int32)
    out["acked"][:] = np.where(ok0, np.maximum(out["acked"].reshape(-1), ack), out["acked"].reshape(-1)).reshape(out["acked"].shape)
    out["requested"][:] = (ok0 & (d0[:, 14 + 5 * P] == 1)).reshape(out["requested"].shape)
    merge = ok0 & (d0[:, 14 + 5 * P] == 0)
    for i in range(P):
        out["last"][:, i] = np.where(merge, u32(d0, 15 + 5 * i).view(np.int32), -1).reshape(out["last"][:, i].shape)
        out["disc"][:, i] = (merge & (d0[:, 14 + 5 * i] == 1)).reshape(out["disc"][:, i].shape)
    out["lengths"][:] = np.where(ok0, plen, 0).astype(np.int32).reshape(out["lengths"].shape)
    out["start"][:] = np.where(ok0, u32(d0, off - 16).view(np.int32), 0).reshape(out["start"].shape)
    out["packets"].reshape(-1, PSTRIDE)[:, :STRIDE - off] = d0[:, off:off + PSTRIDE][:, :STRIDE - off]
    out["advantage"][:] = np.where(ok1, d1[:, 6].view(np.int8), out["advantage"].reshape(-1)).reshape(out["advantage"].shape)
    out["owed"][:] = ok1.reshape(out["owed"].shape)
    out["ping"][0] = np.where(ok1, u64(d1, 7), 0).reshape(out["ping"][0].shape)
    out["ping"][1] = np.where(ok1, u64(d1, 15), 0).reshape(out["ping"][1].shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libggrs_amd.so built from the parent commit")
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=12, help="timed rounds (at least 12)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "datagram_ab.log"))
    args = ap.parse_args()
    if args.rounds < 12:
        raise SystemExit("at least 12 timed rounds")

    import numpy as np
    import torch

    import ggrs_amd as G
    from ggrs_amd import _lib as L
    from time_sync_bench import make_batch, open_lib

    if not torch.cuda.is_available():
        raise SystemExit("datagram_bench needs a GPU: nothing is measured without one")
    S, delay = args.sessions, 2
    n = args.warmup + args.rounds
    dev = torch.device("cuda", 0)
    here, parent = L.load(), open_lib(args.parent_lib)
    stream = torch.cuda.Stream(device=dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    names = ("a1", "b", "c", "d", "cb", "db", "a2", "e")
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for P in (2, 4):
        group = f"p{P}"
        mask = ((1 << P) - 1) & ~1
        remotes = [h for h in range(P) if (mask >> h) & 1]
        T = n + LEAD + BACK + 2
        z = lambda shape, dt, v=0: torch.full(shape, v, dtype=dt, device=dev)
        with torch.cuda.stream(stream):
            dx = torch.from_numpy(G.synth_inputs(S, P, T + delay)).to(dev)
            t = torch.arange(T, dtype=torch.int32, device=dev)
            upto_t = torch.clamp(t - 2, min=-1)[:, None, None].expand(T, P, S).contiguous()
            ring_truth = z((R, P, S), torch.uint8)
            ring_truth[torch.arange(T, device=dev) & (R - 1)] = dx[:T]
            # every round's packets (frames i .. i + BACK against frame i - 1) and datagrams, made once
            pk, ln, st = z((n, P, S, PSTRIDE), torch.uint8), z((n, P, S), torch.int32), z((n, P, S), torch.int32)
            ack = [z((P, S), torch.int32, i - 1) for i in range(n)]
            new = [z((P, S), torch.int32, i + BACK) for i in range(n)]
            dg, dl = z((n, M, P, S, STRIDE), torch.uint8), z((n, M, P, S), torch.int32)
            cnt, bst = z((P, S), torch.int32), z((P, S), torch.int32)
            magic = z((P, S), torch.int16, 0x1234)
            last, disc, ones = z((P, S), torch.int32, 7), z((P, S), torch.uint8), z((P, S), torch.uint8, 1)
            adv = z((P, S), torch.int32, -3)

            def build(i, out_dg, out_ln):
                io = L.RbDatagramBuild(local_magic=p(magic), now_ms=NOW + 16 * i, packets=p(pk[i]), packet_stride=PSTRIDE,
                                       lengths=p(ln[i]), start_frames=p(st[i]), ack_frame=p(ack[i]), status_last_frames=p(last),
                                       status_disconnected=p(disc), report_due=p(ones), frame_advantage=p(adv),
                                       out_datagrams=p(out_dg), stride=STRIDE, slots=M, out_lengths=p(out_ln), out_counts=p(cnt),
                                       status=p(bst))
                assert here.rb_build_datagrams_all(0, sp, mask, P, S, ctypes.byref(io)) == 0

            for i in range(n):
                G.encode_packets(ring_truth, mask, new[i], ack[i], 0, pk[i], ln[i], st[i], ring_frames=R)
                build(i, dg[i], dl[i])
            assert int(ln[:, remotes].min()) > 0 and (cnt[remotes] == 2).all() and (bst[remotes] == 0).all()
            parsed = G.ParsedDatagrams(P, S, PSTRIDE)

            def parse(i):
                o = parsed
                io = L.RbDatagramParse(datagrams=p(dg[i]), stride=STRIDE, slots=M, dg_lengths=p(dl[i]), remote_magic=p(magic),
                                       now_ms=NOW + 16 * i + 5, received=p(o.received), disconnect_requested=p(o.disconnect_requested),
                                       acked=p(o.acked), peer_last_frames=p(o.peer_last_frames), peer_disconnected=p(o.peer_disconnected),
                                       packets=p(o.packets), packet_stride=PSTRIDE, lengths=p(o.lengths), start_frames=p(o.start_frames),
                                       frame_advantage=p(o.frame_advantage), reply_owed=p(o.reply_owed), reply_ping=p(o.reply_ping),
                                       rtt_ms=p(o.rtt_ms), reports=p(o.reports), report_counts=p(o.report_counts), status=p(o.status))
                assert here.rb_parse_datagrams_all(0, sp, mask, P, S, ctypes.byref(io)) == 0

            ring = G.DeliveryRing(R, P, S)
            dstatus = z((P, S), torch.int32)
            enc = (z((P, S, PSTRIDE), torch.uint8), z((P, S), torch.int32), z((P, S), torch.int32))
            bdg, bdl = z((M, P, S, STRIDE), torch.uint8), z((M, P, S), torch.int32)
            # e's host side: pinned arrays and their device twins
            shapes = {"received": ((P, S), np.uint8), "requested": ((P, S), np.uint8), "acked": ((P, S), np.int32),
                      "last": ((P, P, S), np.int32), "disc": ((P, P, S), np.uint8), "lengths": ((P, S), np.int32),
                      "start": ((P, S), np.int32), "packets": ((P, S, PSTRIDE), np.uint8), "advantage": ((P, S), np.int32),
                      "owed": ((P, S), np.uint8), "ping": ((2, P, S), np.uint64)}
            pinned = {k: torch.zeros(sh, dtype=getattr(torch, np.dtype(dt).name if dt != np.uint64 else "int64")).pin_memory()
                      for k, (sh, dt) in shapes.items()}
            host = {k: (v.numpy().view(np.uint64) if k == "ping" else v.numpy()) for k, v in pinned.items()}
            host["acked"][:] = -1
            twin = {k: v.to(dev) for k, v in pinned.items()}
            h_dg = torch.zeros((M, P, S, STRIDE), dtype=torch.uint8).pin_memory()
            h_ln = torch.zeros((M, P, S), dtype=torch.int32).pin_memory()

            batch = {k: make_batch(parent if k in ("a1", "a2") else here, S, P, delay) for k in ("a1", "b", "a2", "pad")}
            for b in batch.values():
                b.set_stream(stream)
                b.run_ticks(dx[:LEAD], upto_t[:LEAD], dx)
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2 * len(names))] for _ in range(n)]
            for i in range(n):
                a = LEAD + i
                for j, k in enumerate(names):
                    ev[i][2 * j].record(stream)
                    if k in ("a1", "b", "a2"):
                        batch[k].run_ticks(dx[a:a + 1], upto_t[a:a + 1], dx)
                    elif k == "c":
                        parse(i)
                    elif k == "d":
                        assert here.rb_decode_input_packets_all(0, sp, mask, P, S, 1, W, p(pk[i]), PSTRIDE, p(ln[i]), p(st[i]),
                                                                p(ring.inputs), R, R, p(ring.upto), p(dstatus)) == 0
                    elif k == "cb":
                        build(i, bdg, bdl)
                    elif k == "db":
                        assert here.rb_encode_input_packets_all(0, sp, mask, P, S, 1, p(ring_truth), R, R, 0, p(ack[i]), p(new[i]),
                                                                p(enc[0]), PSTRIDE, p(enc[1]), p(enc[2])) == 0
                    else:
                        h_dg.copy_(dg[i], non_blocking=True)
                        h_ln.copy_(dl[i], non_blocking=True)
                        stream.synchronize()
                        host_parse(np, h_dg.numpy()[:, 1:], h_ln.numpy()[:, 1:], P, 0x1234,  # the remote handles' rows, as views
                                   {k2: (v[:, 1:] if k2 == "ping" else v[1:]) for k2, v in host.items()})
                        for k2, v in pinned.items():
                            twin[k2].copy_(v, non_blocking=True)
                    ev[i][2 * j + 1].record(stream)
                for _ in range(PADS):
                    batch["pad"].run_ticks(dx[a:a + 1], upto_t[a:a + 1], dx)
            torch.cuda.synchronize()
            us = {k: [ev[i][2 * j].elapsed_time(ev[i][2 * j + 1]) * 1e3 for i in range(args.warmup, n)] for j, k in enumerate(names)}
            # every line did its work, and e's numpy parse agrees with the kernel's
            assert all((batch[k].status()[0] == 0).all() for k in ("a1", "b", "a2"))
            assert batch["b"].totals()[:3] == batch["a1"].totals()[:3]
            top = n - 1 + BACK
            assert (ring.upto[remotes] == top).all() and (parsed.status[remotes] == 0).all() and (parsed.received[remotes] == 1).all()
            for a_, b_ in (("acked", "acked"), ("lengths", "lengths"), ("start", "start_frames"), ("advantage", "frame_advantage"),
                           ("owed", "reply_owed"), ("last", "peer_last_frames"), ("disc", "peer_disconnected"), ("ping", "reply_ping")):
                x, y = twin[a_], getattr(parsed, b_)
                assert torch.equal(x[:, remotes] if a_ == "ping" else x[remotes], y[:, remotes] if a_ == "ping" else y[remotes]), a_
            live = torch.arange(PSTRIDE, device=dev)[None, None, :] < parsed.lengths[remotes][:, :, None]
            assert torch.equal(twin["packets"][remotes][live], parsed.packets[remotes][live])
            assert torch.equal(parsed.packets[remotes][live], pk[n - 1][remotes][live]) and torch.equal(enc[1][remotes], ln[n - 1][remotes])
            assert torch.equal(bdl, dl[n - 1])
            for b in batch.values():
                b.close()
        med = {k: statistics.median(v) for k, v in us.items()}
        base = us["a1"] + us["a2"]
        bm = statistics.median(base)
        bd = mad(base, bm)
        for k in names:
            say(f"{group:4s} {k:3s} median {med[k]:9.2f} us per call  MAD {mad(us[k], med[k]):6.2f}  min {min(us[k]):9.2f}  max {max(us[k]):9.2f}")
        diff = med["b"] - bm
        word = "loss" if diff > 3 * bd else ("gain" if diff < -3 * bd else "within the spread")
        say(f"{group:4s} parent (a1, a2 pooled) median {bm:.2f} us, MAD {bd:.2f}, a1 against a2 {med['a1'] - med['a2']:+.2f} us")
        say(f"{group:4s} b vs parent: {diff:+.2f} us ({diff / bm * 100:+.2f}%): {word} (3 MAD = {3 * bd:.2f} us)")
        say(f"{group:4s} c - d (parse against rb_decode_input_packets_all): {med['c'] - med['d']:+.2f} us; "
            f"cb - db (build against rb_encode_input_packets_all): {med['cb'] - med['db']:+.2f} us (reported, not judged)")
        say(f"{group:4s} e / c (the numpy parse and its copies against the kernel): {med['e'] / med['c']:.1f} times (reported, not judged)")
        results.append({"group": group, "num_players": P, **{f"{k}_us": round(med[k], 2) for k in names}, "parent_us": round(bm, 2),
                        "parent_mad_us": round(bd, 2), "b_minus_parent_us": round(diff, 2), "verdict": word,
                        "c_minus_d_us": round(med["c"] - med["d"], 2), "cb_minus_db_us": round(med["cb"] - med["db"], 2),
                        "e_over_c": round(med["e"] / med["c"], 1)})

    say(json.dumps({"bench": "datagram_bench", "game": "ex_game", "sessions": S, "slots": M, "stride": STRIDE,
                    "timed_rounds": args.rounds, "warmup_rounds": args.warmup, "device": torch.cuda.get_device_name(0),
                    "results": results}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if any(r["verdict"] == "loss" for r in results) else 0


if __name__ == "__main__":
    sys.exit(main())
