"""bench.py's plain run and --dump-outputs.

CPU: bench.main() against the stand-in backend (tests/bench_standin.py): a plain run is set-up, warm-up, the timed steps and
the line -- no events leg, no roofline objects, no extra legs, which --full adds; --dump-outputs writes float arrays of the
last timed step, the same from run to run.
GPU: the real backend's dump of a small run is the oracle's opcode stream of the sampled clips, bit for bit."""

import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONTRACT_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")


def _main(monkeypatch, argv):
    import bench
    from bench_standin import CpuStandIn
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    made = []

    def factory(args, local_rank, world):
        made.append(CpuStandIn(args, local_rank, world))
        return made[-1]

    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = bench.main(["--frames-per-step", "4", "--streams", "64"] + argv, backend_cls=factory)
    lines = [l for l in buf.getvalue().splitlines() if l.strip()]
    assert len(lines) == 1 and json.loads(lines[0]) == json.loads(json.dumps(out))
    return out, made[0].log


def test_plain_run_is_warmup_and_timed_steps_only(monkeypatch):
    out, log = _main(monkeypatch, ["--steps", "5", "--warmup", "2"])
    assert log["steps"] == 2 + 5 and log["checks"] == 2          # no events leg
    for k in CONTRACT_KEYS:
        assert k in out
    assert out["steps"] == 5 and out["warmup"] == 2 and out["full"] is False
    assert out["value"] == pytest.approx(5 * 4 * 64 * 1000.0 / (out["ms_per_step"] * 5))
    for k in ("roofline", "roofline_prologue", "kernel_time_share", "events_leg", "access_pattern_reference"):
        assert k not in out


def test_full_run_adds_the_events_leg_and_roofline(monkeypatch):
    out, log = _main(monkeypatch, ["--steps", "5", "--warmup", "2", "--full"])
    assert log["steps"] == 2 + 3 + 5 and log["checks"] == 3
    assert out["full"] is True and out["events_leg"]["steps"] == 3
    assert "roofline" in out and "roofline_prologue" in out and "kernel_time_share" in out


def test_dump_outputs_are_float_bounded_and_repeatable(monkeypatch, tmp_path):
    got = []
    for d in ("a", "b"):
        out, log = _main(monkeypatch, ["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / d)])
        assert out["dumped_outputs"]["names"] == ["opcode_streams", "segments"]
        files = sorted(os.listdir(tmp_path / d))
        assert files == ["opcode_streams.npy", "segments.npy"]
        arrays = {f: np.load(tmp_path / d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        got.append(arrays)
    for f in got[0]:
        assert np.array_equal(got[0][f], got[1][f])
    import stream_batch
    clock = stream_batch.MovieClock(True)
    last = [clock.segments(4) for _ in range(1 + 3)][-1]            # the last TIMED step's segments
    assert np.array_equal(got[0]["segments.npy"], np.asarray(last, np.float64))


def test_dump_sample_is_fixed_and_within_the_limit():
    import bench
    per_stream = 50 * 490 * 6 * 4                                   # the default step's opcode rows of one stream, float32
    a, b = bench.dump_sample(14336, per_stream), bench.dump_sample(14336, per_stream)
    assert np.array_equal(a, b) and len(a) == 64 and len(set(a.tolist())) == 64 and a.max() < 14336
    assert len(a) * per_stream <= bench.DUMP_MAX_BYTES
    assert np.array_equal(bench.dump_sample(8, per_stream), np.arange(8))
    assert len(bench.dump_sample(14336, 20 * per_stream)) * 20 * per_stream <= bench.DUMP_MAX_BYTES


def test_cli_plain_run_with_dump(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "tests"), os.path.join(ROOT, "ii-vision_amd", "transcoder"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--frames-per-step", "4", "--streams", "8", "--backend", "bench_standin:CpuStandIn",
                        "--dump-outputs", str(tmp_path / "out")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and "roofline" not in d
    assert sorted(os.listdir(tmp_path / "out")) == ["opcode_streams.npy", "segments.npy"]


@pytest.mark.gpu
def test_bench_dump_is_the_oracle_stream(tmp_path, O, oracle_tables):
    """A plain DHGR run of 96 clips, one warm-up and two timed steps of 10 frames: the dumped rows of the last timed step are
    the oracle's opcodes for those clips -- same synthetic input, same seeds, the clip wrapping as the bench's does."""
    import bench
    import stream_batch
    S, W, K, F = 96, 1, 2, 10
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "IIV_BENCH_REHEARSE_ON_ONE_GPU")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--streams", str(S), "--steps", str(K),
                        "--warmup", str(W), "--frames-per-step", str(F), "--dump-outputs", str(tmp_path / "out")],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.strip()][-1])
    assert d["steps"] == K and d["ms_per_step"] > 0 and "roofline" not in d and d["config"]["streams_per_gpu"] == S
    ops = np.load(tmp_path / "out" / "opcodes.npy")
    streams = np.load(tmp_path / "out" / "opcode_streams.npy")
    segs = np.load(tmp_path / "out" / "segments.npy")
    assert ops.dtype == np.float32 and streams.dtype == np.float64 and segs.dtype == np.float64
    assert np.array_equal(streams, bench.dump_sample(S, ops.shape[1] * 6 * 4).astype(np.float64)) and len(streams) == 64
    clock = stream_batch.MovieClock(True)
    steps = [clock.segments(F) for _ in range(W + K)]
    assert np.array_equal(segs, np.asarray(steps[-1], np.float64))
    assert ops.shape == (64, sum(s[3] for s in steps[-1]), 6)
    fm, fa = stream_batch.synth_frames_torch(S, K * F, True, seed=bench.data_seed(0))
    seeds = bench.rank_seeds(0, S)
    for i in (0, 31, 63):
        s = int(streams[i])
        main, aux = fm[s].cpu().numpy(), fa[s].cpu().numpy()
        v = O.Video(1, oracle_tables.get(1), seed_py=seeds[s][0], seed_np=seeds[s][1])
        for j, step in enumerate(steps):
            exp = []
            for (f, ia, restart, k) in step:
                if restart:
                    v.encode_frame(main[f % (K * F)], aux[f % (K * F)], ia)
                exp.append(v.next(k))
        assert np.array_equal(ops[i], np.concatenate(exp).astype(np.float32)), "stream %d" % s
