"""A spectator batch's launch against a P2P batch's launch of the same shape, in one process.

A spectator tick does a strict subset of a P2P tick's work (no prediction, no rollback, no
cells), so a spectator launch must not take longer than the P2P launch measured next to it.
Shape: ex_game, 2 players, 65,536 sessions, 50 ticks per launch.  Every delivery lags by one
tick (synth_network's lag 1: what a peer made in its tick k arrives before tick k + 2), so
neither side starves: the P2P sessions predict the remote player's last two frames and roll
back when a held input changed, the spectators advance one frame per tick.  Both batches run
on one stream, launches alternate, each between its own pair of device events.

    python3 tools/spectator_bench.py [--launches 12] [--out profiles/spectator_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--ticks-per-launch", type=int, default=50)
    ap.add_argument("--launches", type=int, default=12, help="timed launches of each batch (at least 10)")
    ap.add_argument("--warmup", type=int, default=3, help="untimed launches of each batch before them")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectator_bench.json"))
    args = ap.parse_args()
    if args.launches < 10:
        raise SystemExit("at least 10 timed launches")

    import torch

    import ggrs_amd as G
    from ggrs_amd.p2p import PlayerType

    if not torch.cuda.is_available():
        raise SystemExit("spectator_bench needs a GPU: nothing is measured without one")
    S, P, tpl, delay = args.sessions, 2, args.ticks_per_launch, 2
    n = args.warmup + args.launches
    T = n * tpl
    dev = torch.device("cuda", 0)
    x = G.synth_inputs(S, P, T + delay)  # [frames, P, S]
    dx = torch.from_numpy(x).to(dev)
    t = torch.arange(T, dtype=torch.int32, device=dev)
    # lag 1 (ggrs_amd.p2p.synth_network: t - 1 - lag): before tick t the newest frame delivered is
    # t - 2, for the host's remote handle (handle 0 is local, input delay 2) and for the spectators
    lagged = torch.clamp(t - 2, min=-1)
    p2p_upto = lagged[:, None, None].expand(T, P, S).contiguous()
    spec_upto = lagged[:, None].expand(T, S).contiguous()

    b = G.SessionBuilder(G.Game.EX_GAME, num_sessions=S).with_num_players(P).with_input_delay(delay)
    b.add_player(PlayerType.Local, 0).add_player(PlayerType.Remote, 1)
    host = b.start_p2p_session()
    spec = G.SessionBuilder(G.Game.EX_GAME, num_sessions=S).with_num_players(P).start_spectator_session()
    stream = torch.cuda.Stream(device=dev)
    host.set_stream(stream)
    spec.set_stream(stream)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(n)]
    with torch.cuda.stream(stream):
        for i in range(n):
            a, z = i * tpl, (i + 1) * tpl
            ev[i][0].record(stream)
            host.run_ticks(dx[a:z], p2p_upto[a:z], dx)
            ev[i][1].record(stream)
            spec.run_ticks(spec_upto[a:z], dx)
            ev[i][2].record(stream)
        torch.cuda.synchronize()
    p2p_us = [ev[i][0].elapsed_time(ev[i][1]) * 1e3 for i in range(args.warmup, n)]
    spec_us = [ev[i][1].elapsed_time(ev[i][2]) * 1e3 for i in range(args.warmup, n)]

    # both sides did the work the shape promises
    st = host.status()[0]
    cur, _ = host.frames()
    assert (st == 0).all() and (cur == T).all(), "the P2P sessions must advance every tick"
    adv, saves, loads = host.totals()[:3]
    assert loads > 0, "the P2P sessions must roll back"
    sst, _ = spec.status()
    scur, srecv = spec.frames()
    sadv, thr, far = spec.totals()
    assert (sst == 0).all() and (scur == T - 3).all() and (srecv == T - 3).all()
    assert sadv == S * (T - 2) and thr == 2 * S and far == 0  # only ticks 0 and 1 wait

    p, s = statistics.median(p2p_us), statistics.median(spec_us)
    res = {
        "bench": "spectator_bench", "game": "ex_game", "num_players": P, "sessions": S, "ticks_per_launch": tpl,
        "timed_launches": args.launches, "warmup_launches": args.warmup, "lag_frames": 1,
        "timing": "device events around each launch, launches alternating on one stream",
        "p2p_us_per_launch": round(p, 2), "spectator_us_per_launch": round(s, 2), "ratio": round(s / p, 4),
        "p2p_us": [round(v, 2) for v in p2p_us], "spectator_us": [round(v, 2) for v in spec_us],
        "p2p_advance_frames": adv, "p2p_load_game_states": loads, "spectator_advance_frames": sadv,
        "device": torch.cuda.get_device_name(0),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("p2p_us_per_launch", "spectator_us_per_launch", "ratio")}))
    host.close()
    spec.close()
    if s > p:
        raise SystemExit(f"a spectator launch ({s:.1f} us) took longer than the P2P launch ({p:.1f} us)")


if __name__ == "__main__":
    main()
