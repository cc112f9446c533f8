"""bench.py --dump-outputs / --full: the dump's formats, budget and seeded row sample (CPU, on host arrays), and on
the GPU one small plain run whose dumped arrays are the oracle's and whose line carries no leg of --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _arrays(n, h):
    rng = np.random.default_rng(5)
    return dict(views=rng.integers(0, 1 << 40, n, dtype=np.uint64), flags=rng.integers(0, 1 << 31, n).astype(np.uint32),
                round=rng.integers(0, 1 << 16, (n, h)).astype(np.uint16),
                time_tick=rng.integers(0, 1 << 32, (n, h)).astype(np.uint32),
                block_hash=rng.integers(0, 256, (n, h, 32)).astype(np.uint8))


def test_dump_whole_when_it_fits(tmp_path):
    import bench
    a = _arrays(64, 10)
    bench.dump_outputs(str(tmp_path), 0, a)
    assert sorted(os.listdir(tmp_path)) == sorted(f"{k}.npy" for k in a)      # no sample_rows.npy
    for k, v in a.items():
        got = np.load(tmp_path / f"{k}.npy")
        assert got.dtype == (np.float32 if v.dtype.itemsize <= 2 else np.float64) and got.shape == v.shape
        assert np.array_equal(got.astype(v.dtype), v)                         # exact in the float format


def test_dump_samples_rows_within_budget(tmp_path):
    import bench
    a = _arrays(16_384, 100)
    bench.dump_outputs(str(tmp_path / "a"), 0, a)
    bench.dump_outputs(str(tmp_path / "b"), 3, a)                             # rank 3: its own directory
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b" / "rank3")) and "sample_rows.npy" in files
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) < 64_000_000
    rows = np.load(tmp_path / "a" / "sample_rows.npy").astype(np.int64)
    assert np.array_equal(rows, np.load(tmp_path / "b" / "rank3" / "sample_rows.npy"))   # the same rows every time
    assert 1024 < len(rows) < 16_384 and (np.diff(rows) > 0).all()
    for k, v in a.items():
        got = np.load(tmp_path / "a" / f"{k}.npy")
        assert np.array_equal(got.astype(v.dtype), v if v.ndim == 1 else v[rows])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path):
    """256 cfg3 instances x 10 heights, 3 timed steps: every dumped array equals the oracle's, the line says what
    was timed, and a run without --full carries no CPU baseline."""
    import oracle_lib as O
    from bftsim.configs import cfg3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--instances", "256", "--heights", "10", "--dump-outputs", str(tmp_path / "d")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and "cpu_baseline" not in out
    ref = O.run(cfg3(heights=10), 0, 256)
    assert out["value"] == pytest.approx(int(ref["views"].sum()) / (out["ms_per_step"] / 1e3))
    assert not (tmp_path / "d" / "sample_rows.npy").exists()
    for k in ("committed_height", "flags", "ticks", "views", "round", "proposer", "variant", "time_tick", "block_hash"):
        got = np.load(tmp_path / "d" / f"{k}.npy")
        assert got.dtype in (np.float32, np.float64) and np.array_equal(got.astype(ref[k].dtype), ref[k]), k
