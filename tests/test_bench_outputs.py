"""bench.py --dump-outputs: the files hold the state the timed path left after
its last timed tick, and a plain run does none of the --full work."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_outputs_samples_the_same_sessions_within_the_budget(tmp_path):
    bench = _bench_module()
    S, B = 6000, 8192  # 6000 x 2048 words as float64 = 98 MB: sampled
    img = np.zeros((S, B), np.uint8)
    img[:, :4] = np.arange(S, dtype=np.int32).view(np.uint8).reshape(S, 4)
    extra = {"display_checksum": np.arange(S, dtype=np.uint64) * 3}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), "brawler", 2, img, extra, seed=7)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["display_checksum.npy", "sessions.npy", "state_words.npy"]
    got = {f: np.load(tmp_path / "a" / f) for f in files}
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_BUDGET_BYTES < 64 << 20
    assert all(a.dtype == np.float64 for a in got.values())
    keep = got["sessions.npy"].astype(np.int64)
    assert 0 < len(keep) < S and (np.diff(keep) > 0).all()
    assert (got["state_words.npy"][:, 0] == keep).all() and (got["display_checksum.npy"] == 3 * keep).all()
    for f in files:  # the same seed keeps the same sessions
        assert np.array_equal(got[f], np.load(tmp_path / "b" / f))


def test_dump_outputs_splits_ex_game_into_f32_fields(tmp_path):
    bench = _bench_module()
    S, P = 33, 2
    words = np.zeros((S, 9 + 5 * P), np.float32)  # bincode image: 36 + 20 P bytes
    words[:, 5:5 + 2 * P] = np.arange(S * 2 * P, dtype=np.float32).reshape(S, 2 * P) + 0.5  # positions at byte 20
    img = words.view(np.uint8)
    bench.dump_outputs(str(tmp_path), "ex_game", P, img, {}, seed=1)
    pos = np.load(tmp_path / "positions.npy")
    assert pos.dtype == np.float32 and pos.shape == (S, P, 2)
    assert np.array_equal(pos.reshape(S, 2 * P), words[:, 5:5 + 2 * P])
    assert np.array_equal(np.load(tmp_path / "sessions.npy"), np.arange(S))
    assert {"frame.npy", "velocities.npy", "rotations.npy"} <= set(os.listdir(tmp_path))


@pytest.mark.gpu
def test_gpu_plain_bench_run_dumps_the_last_timed_tick(gpu_available, tmp_path):
    import ggrs_amd as G

    S, P, steps, warmup, cd = 320, 2, 6, 3, 7
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--sessions-per-gpu", str(S), "--ticks-per-launch", "4", "--dump-outputs",
                        str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["cpu_baseline"] is None and d["realtime"] is None and d["roofline"]["measured_copy_GBps"] is None
    # the same ticks through a batch of this process: start-up, warmup and timed ticks, nothing after
    T = cd + 1 + warmup + steps
    inputs = G.synth_inputs(S, P, T, seed=0x67677273)
    sess = (G.SessionBuilder(G.Game.EX_GAME, num_sessions=S, device=0).with_num_players(P)
            .with_check_distance(cd).with_input_delay(2).start_synctest_session())
    sess.run_ticks(inputs)
    img, dcs, dfr = sess.read_live()
    sess.close()
    want = G.session.decode_ex_game(img, P)
    assert (np.load(tmp_path / "frame.npy") == T).all() and (want["frame"] == T).all()
    for k in ("positions", "velocities", "rotations"):
        got = np.load(tmp_path / f"{k}.npy")
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want[k].view(np.uint32)), k
    assert np.array_equal(np.load(tmp_path / "display_checksum.npy"), dcs.astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "display_frame.npy"), dfr.astype(np.float64))
    assert (np.load(tmp_path / "mismatch_frame.npy") == G.NULL_FRAME).all()
