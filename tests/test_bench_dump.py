"""bench.py --dump-outputs / --full: the dump helper on synthetic batches
(CPU), and one tiny end-to-end bench run on the GPU checked for run-to-run
identical dumps and a lean result line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def _batch(keys, w_end, rng):
    n = len(keys)
    names = [f"sensor_{k}".encode() for k in keys]
    offs = np.zeros(n + 1, np.int32)
    np.cumsum([len(x) for x in names], out=offs[1:])
    return {
        "n_rows": n,
        "key_offsets": offs,
        "key_data": np.frombuffer(b"".join(names), np.uint8),
        "count": rng.integers(1, 900, n).astype(np.int64),
        "max": rng.uniform(113, 115, n),
        "valid": np.ones(n, np.uint8),
        "window_start": np.full(n, w_end - 1000, np.int64),
        "window_end": np.full(n, w_end, np.int64),
    }


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _keys(cols):
    o = cols["key_offsets"].astype(np.int64)
    raw = cols["key_data"].astype(np.uint8).tobytes()
    return [raw[o[i]:o[i + 1]].decode() for i in range(len(o) - 1)]


def test_dump_keeps_only_last_step_windows(tmp_path):
    rng = np.random.default_rng(1)
    # an early window (closed by a previous step, polled late) then two of
    # the last step's; one batch mixes both kinds
    b0 = _batch([5, 17, 123], 9000, rng)
    b1 = _batch([17, 4000], 10000, rng)
    b1["window_end"][0] = 9000
    b2 = _batch([9, 10, 11], 11000, rng)
    n, sampled = bench.dump_outputs(str(tmp_path), [b0, b1, b2], 9000, 42, 0, 1)
    assert (n, sampled) == (4, False)
    cols = _load(str(tmp_path))
    assert set(cols) == {"key_offsets", "key_data", "count", "max", "valid",
                         "window_start", "window_end"}
    for k, v in cols.items():
        assert v.dtype in (np.float32, np.float64), k
    assert _keys(cols) == ["sensor_4000", "sensor_9", "sensor_10", "sensor_11"]
    assert np.array_equal(cols["count"],
                          np.concatenate([b1["count"][1:], b2["count"]]))
    assert np.array_equal(cols["max"],
                          np.concatenate([b1["max"][1:], b2["max"]]))
    assert np.array_equal(cols["window_end"], [10000, 11000, 11000, 11000])


def test_dump_int_keys_and_empty(tmp_path):
    rng = np.random.default_rng(2)
    b = _batch([1, 2], 5000, rng)
    del b["key_offsets"], b["key_data"]
    b["key"] = np.array([1, 2], np.int64)
    assert bench.dump_outputs(str(tmp_path / "a"), [b], 0, 42, 0, 1) == (2, False)
    assert np.array_equal(_load(str(tmp_path / "a"))["key"], [1.0, 2.0])
    # nothing of the last step in the polls: arrays exist, all empty
    assert bench.dump_outputs(str(tmp_path / "b"), [b], 5000, 42, 0, 1) == (0, False)
    assert all(len(v) == 0 for v in _load(str(tmp_path / "b")).values())


def test_dump_sample_is_seeded_and_bounded(tmp_path, monkeypatch):
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 10_000, 5000)
    b = _batch(keys, 2000, rng)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 64 << 10)
    r1 = bench.dump_outputs(str(tmp_path / "a"), [b], 0, 7, 0, 1)
    r2 = bench.dump_outputs(str(tmp_path / "b"), [b], 0, 7, 0, 1)
    assert r1 == r2 and r1[1] and 0 < r1[0] < 5000
    a, c = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(v.nbytes for v in a.values()) <= 80 << 10
    for k in a:
        assert np.array_equal(a[k], c[k]), k
    idx = a["sample_row_index"].astype(np.int64)
    assert np.all(np.diff(idx) > 0)
    assert np.array_equal(a["count"], b["count"][idx])
    assert _keys(a) == [f"sensor_{k}" for k in keys[idx]]


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dump_repeats(tmp_path):
    def run(d, *extra):
        r = subprocess.run(
            [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
             "--steps", "3", "--warmup", "1", "--rows-per-step", "300000",
             "--keys", "257", "--dump-outputs", str(d), *extra],
            capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.strip().splitlines()
        assert len(lines) == 1
        return json.loads(lines[0]), _load(str(d))

    res, a = run(tmp_path / "a")
    assert res["steps"] == 3 and res["ms_per_step"] > 0
    assert abs(res["value"] - 300000 / (res["ms_per_step"] / 1e3)) \
        <= 1e-6 * res["value"]
    assert res["cpu_baseline"] is None  # only with --full
    # the last step's rows start at 1_000_000 + 900 ms of stream: only
    # windows still open then belong to it, and finish() flushes them
    assert len(a["count"]) > 0
    assert np.all(a["window_end"] > 1_000_000 + 900)
    assert np.all(a["max"] > 113.0)
    _, b = run(tmp_path / "b")
    # room for 2 of the 4 steps only: the inputs are regenerated in place
    # mid-run, which must not change what the steps compute
    res_c, c = run(tmp_path / "c", "--resident-gib", "0.02")
    assert res_c["steps"] == 3 and res_c["ms_per_step"] > 0
    for other in (b, c):
        assert set(a) == set(other)
        for k in a:
            assert np.array_equal(a[k], other[k]), k
