"""What one rb_endpoint_protocol_poll_all costs, against the parent commit's library, in one process.

Shapes: ex_game, 2 and 4 players (handle 0 local), 65,536 sessions.  The lines of a group run on one
stream, their calls alternating, each between its own pair of device events, with the parent commit's
library first and last in every round; 3 warm-up rounds, medians of 12.  Every line calls the C entry
points through ctypes:

    a1, a2  one-tick rb_p2p_run_ticks of the parent commit's library (--parent-lib); two of them, so
            the run shows what the same code measures against itself
    b       this tree's one-tick rb_p2p_run_ticks (no tick kernel changed: within the band)
    c       one rb_endpoint_protocol_poll_all over every remote endpoint, all Running, two incoming
            slots (an Input and a QualityReport, neither a sync kind), two sync slots, every optional
            tensor given: the steady state of a match
    h       the same call while every endpoint shakes hands: a SyncReply to the outstanding nonce in
            slot 0, so each endpoint removes a nonce, inserts one and writes a SyncRequest
    d       rb_parse_datagrams_all over c's datagrams: the call that runs just before it in the frame loop
    e       c's decisions as a caller makes them today: the state rows copied to the host, the timers
            and counters in numpy over all P x S endpoints, the outputs copied back (it synchronises, so
            it runs after a2, outside the judged part of the round, and PADS untimed calls follow it)

The rule is tools/ab.py's: b against the parent counts as a loss (or a gain) only beyond three times
the parent's own median absolute deviation (a1 and a2 pooled).  c, h, c - d and e / c are reported,
not judged.

    python3 tools/protocol_bench.py --parent-lib /path/to/parent/libggrs_amd.so
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
STRIDE, PSTRIDE, M, Q = 64, 32, 2, 2
PADS, LEAD = 8, 3
NOW = 1_700_000_000_000


def mad(v, m):
    return statistics.median(abs(x - m) for x in v)


def host_poll(np, st, now, received, ack_owed, reply_owed, newest, acked, lengths, out):
    """c's decisions for Running endpoints with numpy: steps 5 to 9 of the header over [P, S] arrays."""
    last_send, last_input, last_report = st["stamps"][0], st["stamps"][1], st["stamps"][2]
    running = st["ep_state"] == 2
    ack = running & (ack_owed != 0)
    last_input[ack] = now
    reply = running & (reply_owed != 0)
    resend = running & (last_input + 200 < now)
    last_input[resend] = now
    inp = resend & (newest > acked)
    report = running & (last_report + 200 < now)
    last_report[report] = now
    fresh = running & (newest + 1 > st["last_newest"])
    st["last_newest"][fresh] = newest[fresh] + 1
    inp |= fresh
    due = ack.astype(np.int64) + reply + report + inp
    keep = running & (due == 0) & (last_send + 200 < now)
    due += keep
    st["packets_sent"] += due
    last_send[due > 0] = now
    out["input_lengths"][:] = np.where(inp, lengths, 0)
    out["ack_due"][:], out["reply_due"][:], out["report_due"][:], out["keepalive_due"][:] = ack, reply, report, keep
    out["liveness_received"][:] = (received != 0) | ~running
    out["send_queue_len"][:] = np.maximum(newest - acked, 0)
    out["session_running"][:] = (st["ep_state"][1:] >= 2).all(axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libggrs_amd.so built from the parent commit")
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=12, help="timed rounds (at least 12)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "protocol_ab.log"))
    args = ap.parse_args()
    if args.rounds < 12:
        raise SystemExit("at least 12 timed rounds")

    import numpy as np
    import torch

    import ggrs_amd as G
    from ggrs_amd import _lib as L
    from time_sync_bench import make_batch, open_lib

    if not torch.cuda.is_available():
        raise SystemExit("protocol_bench needs a GPU: nothing is measured without one")
    S, delay = args.sessions, 2
    n = args.warmup + args.rounds
    dev = torch.device("cuda", 0)
    here, parent = L.load(), open_lib(args.parent_lib)
    stream = torch.cuda.Stream(device=dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    names = ("a1", "b", "c", "h", "d", "a2", "e")
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for P in (2, 4):
        group = f"p{P}"
        mask = ((1 << P) - 1) & ~1
        remotes = [h for h in range(P) if (mask >> h) & 1]
        T = n + LEAD + 2
        z = lambda shape, dt, v=0: torch.full(shape, v, dtype=dt, device=dev)
        with torch.cuda.stream(stream):
            dx = torch.from_numpy(G.synth_inputs(S, P, T + delay)).to(dev)
            t = torch.arange(T, dtype=torch.int32, device=dev)
            upto_t = torch.clamp(t - 2, min=-1)[:, None, None].expand(T, P, S).contiguous()
            magic, peer_magic = z((P, S), torch.int16, 0x1234), 0x4321
            # c's datagrams: an Input's head and a QualityReport, as the wire has them (variants 2 and 4)
            dg, dl = z((M, P, S, STRIDE), torch.uint8), z((M, P, S), torch.int32)
            for m, (variant, length) in enumerate(((2, 31 + 5 * P + 3), (4, 23))):
                dg[m, :, :, 0], dg[m, :, :, 1], dg[m, :, :, 2] = peer_magic & 0xFF, peer_magic >> 8, variant
                dl[m] = length
            dg[0, :, :, 6] = P
            nonces = torch.randint(-2**31, 2**31, (n + 1, M, P, S), dtype=torch.int32, device=dev)
            ones, zeros8 = z((P, S), torch.uint8, 1), z((P, S), torch.uint8)
            lengths = z((P, S), torch.int32, 9)
            newest = [z((P, S), torch.int32, i + 2) for i in range(n)]
            acked = [z((P, S), torch.int32, i - 1) for i in range(n)]
            reports = z((L.RB_P2P_REPORTS_PER_TAKE, S, 3), torch.int64)
            reports[:, :, 2] = -1
            run_ep = G.EndpointProtocol(P, S, dev, Q)
            run_ep.ep_state.fill_(L.RB_EP_RUNNING)
            run_ep.stamps.fill_(NOW)
            run_ep.remote_magic.fill_(peer_magic)
            shake_ep = G.EndpointProtocol(P, S, dev, Q)
            for ep in (run_ep, shake_ep):
                ep.sync_datagrams = z((Q, P, S, STRIDE), torch.uint8)
            # h's datagrams: round i answers the nonce round i - 1 sent (round 0 starts the handshake)
            hdg, hdl = z((n, M, P, S, STRIDE), torch.uint8), z((n, M, P, S), torch.int32)
            hdg[:, 0, :, :, 0], hdg[:, 0, :, :, 1], hdg[:, 0, :, :, 2] = peer_magic & 0xFF, peer_magic >> 8, 1
            for i in range(1, n):
                hdg[i, 0, :, :, 6:10] = nonces[i - 1, 0].view(torch.uint8).view(P, S, 4)
                hdl[i, 0] = 10

            def poll(ep, i, datagrams, dg_lengths, steady):
                io = L.RbEndpointProtocol(
                    **{k: p(getattr(ep, k)) for k in ("ep_state", "sync_remaining", "sync_nonces", "sync_valid", "sync_next",
                                                       "stamps", "packets_sent", "last_newest", "remote_magic")},
                    now_ms=NOW + 16 * i, local_magic=p(magic), start=p(ones), datagrams=p(datagrams), stride=STRIDE, slots=M,
                    sync_slots=Q, dg_lengths=p(dg_lengths), nonces=p(nonces[i]), disconnected=p(zeros8),
                    ack_owed=p(ones if steady else zeros8), reply_owed=p(zeros8), received=p(ones), newest=p(newest[i]),
                    acked=p(acked[i]), lengths=p(lengths), reports=p(reports), input_lengths=p(ep.input_lengths),
                    ack_due=p(ep.ack_due), reply_due=p(ep.reply_due), report_due=p(ep.report_due),
                    keepalive_due=p(ep.keepalive_due), sync_datagrams=p(ep.sync_datagrams), sync_lengths=p(ep.sync_lengths),
                    sync_counts=p(ep.sync_counts), events=p(ep.events_mask), sync_count=p(ep.sync_count),
                    liveness_received=p(ep.liveness_received), send_queue_len=p(ep.send_queue_len),
                    session_running=p(ep.session_running), status=p(ep.status))
                assert here.rb_endpoint_protocol_poll_all(0, sp, mask, P, S, ctypes.byref(io)) == 0

            parsed = G.ParsedDatagrams(P, S, PSTRIDE)

            def parse(i):
                o = parsed
                io = L.RbDatagramParse(datagrams=p(dg), stride=STRIDE, slots=M, dg_lengths=p(dl), remote_magic=p(run_ep.remote_magic),
                                       now_ms=NOW + 16 * i, received=p(o.received), disconnect_requested=p(o.disconnect_requested),
                                       acked=p(o.acked), peer_last_frames=p(o.peer_last_frames), peer_disconnected=p(o.peer_disconnected),
                                       packets=p(o.packets), packet_stride=PSTRIDE, lengths=p(o.lengths), start_frames=p(o.start_frames),
                                       frame_advantage=p(o.frame_advantage), reply_owed=p(o.reply_owed), reply_ping=p(o.reply_ping),
                                       rtt_ms=p(o.rtt_ms), reports=p(o.reports), report_counts=p(o.report_counts), status=p(o.status))
                assert here.rb_parse_datagrams_all(0, sp, mask, P, S, ctypes.byref(io)) == 0

            # e's host side: a twin endpoint set, its state in pinned memory
            host_ep = G.EndpointProtocol(P, S, dev, Q)
            host_ep.ep_state.fill_(L.RB_EP_RUNNING)
            host_ep.stamps.fill_(NOW)
            state_names = ("ep_state", "stamps", "packets_sent", "last_newest")
            out_names = ("input_lengths", "ack_due", "reply_due", "report_due", "keepalive_due", "liveness_received",
                         "send_queue_len", "session_running")
            pin = {k: torch.zeros_like(getattr(host_ep, k), device="cpu").pin_memory() for k in state_names + out_names}
            host = {k: v.numpy() for k, v in pin.items()}
            h_in = {k: v.cpu().numpy() for k, v in (("ones", ones), ("zeros", zeros8), ("lengths", lengths))}

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
                        poll(run_ep, i, dg, dl, True)
                    elif k == "h":
                        poll(shake_ep, i, hdg[i], hdl[i], False)
                    elif k == "d":
                        parse(i)
                    else:
                        for k2 in state_names:
                            pin[k2].copy_(getattr(host_ep, k2), non_blocking=True)
                        stream.synchronize()
                        host_poll(np, host, NOW + 16 * i, h_in["ones"], h_in["ones"], h_in["zeros"], np.full((P, S), i + 2, np.int32),
                                  np.full((P, S), i - 1, np.int32), h_in["lengths"], host)
                        for k2 in state_names + out_names:
                            getattr(host_ep, k2).copy_(pin[k2], non_blocking=True)
                    ev[i][2 * j + 1].record(stream)
                for _ in range(PADS):
                    batch["pad"].run_ticks(dx[a:a + 1], upto_t[a:a + 1], dx)
            torch.cuda.synchronize()
            us = {k: [ev[i][2 * j].elapsed_time(ev[i][2 * j + 1]) * 1e3 for i in range(args.warmup, n)] for j, k in enumerate(names)}
            # every line did its work: the ticks ran, c's endpoints sent an Input and an InputAck every call and
            # a QualityReport when it fell due, as e's numpy says; h's endpoints finished their five round trips
            assert all((batch[k].status()[0] == 0).all() for k in ("a1", "b", "a2"))
            assert batch["b"].totals()[:3] == batch["a1"].totals()[:3]
            for k2 in state_names:
                x, y = getattr(run_ep, k2), getattr(host_ep, k2)
                assert torch.equal(x[..., remotes, :], y[..., remotes, :]), k2
            for k2 in out_names[:-1]:
                assert torch.equal(getattr(run_ep, k2)[remotes], getattr(host_ep, k2)[remotes]), k2
            assert (run_ep.session_running == 1).all() and (run_ep.packets_sent[remotes] >= 2 * n).all()
            assert (shake_ep.ep_state[remotes] == L.RB_EP_RUNNING).all() and (shake_ep.remote_magic[remotes] == peer_magic).all()
            assert (parsed.received[remotes] == 1).all()
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
        say(f"{group:4s} c - d (the protocol call against rb_parse_datagrams_all): {med['c'] - med['d']:+.2f} us; "
            f"h - c (shaking hands against running): {med['h'] - med['c']:+.2f} us (reported, not judged)")
        say(f"{group:4s} e / c (the numpy decisions and their copies against the kernel): {med['e'] / med['c']:.1f} times (reported, not judged)")
        results.append({"group": group, "num_players": P, **{f"{k}_us": round(med[k], 2) for k in names}, "parent_us": round(bm, 2),
                        "parent_mad_us": round(bd, 2), "b_minus_parent_us": round(diff, 2), "verdict": word,
                        "c_minus_d_us": round(med["c"] - med["d"], 2), "e_over_c": round(med["e"] / med["c"], 1)})

    say(json.dumps({"bench": "protocol_bench", "game": "ex_game", "sessions": S, "slots": M, "sync_slots": Q, "stride": STRIDE,
                    "timed_rounds": args.rounds, "warmup_rounds": args.warmup, "device": torch.cuda.get_device_name(0),
                    "results": results}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if any(r["verdict"] == "loss" for r in results) else 0


if __name__ == "__main__":
    sys.exit(main())
