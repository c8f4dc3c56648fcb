"""Cost of int64 value columns: an A/B on one machine, one measurement per
process, one JSON line each. BASELINE.md "Measured: int64 value columns"
reports the set. This is not bench.py.

Shape: cfg2 with dense keys (8M-row steps, 10k keys, 1000 rows/ms, 1 s
tumbling window), the pipelined borrowed push/poll loop of bench.py, wall
time over the timed steps.

  --mode f64       count, min, max, avg over the f64 readings (also runs on a
                   build without int64 values: it names no new symbol)
  --mode f64var    the same plus stddev (the f64 fold with Welford state)
  --mode int64     count, min, max, avg over the same stream's readings
                   scaled by --scale and truncated to int64
  --mode int64var  the same plus stddev

The int64 column is made once, before the warm-up: each step's readings are
read back, scaled, truncated on the host and written to a device buffer of
the same shape. `regfold_ms_per_step` comes from kernel_stats() (HIP events on
every 8th launch, scaled to all launches), over all steps, warm-up included.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import denormalized_amd as dz  # noqa: E402
from denormalized_amd import _lib  # noqa: E402

BASE = ["count", "min", "max", "avg"]


def at(arr, byte_off):
    return ctypes.c_void_p(arr.ptr.value + byte_off)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mode", required=True,
                   choices=["f64", "f64var", "int64", "int64var"])
    p.add_argument("--keys", type=int, default=10_000)
    p.add_argument("--rows", type=int, default=8_000_000)
    p.add_argument("--steps", type=int, default=16)
    p.add_argument("--warmup", type=int, default=4)
    p.add_argument("--rows-per-ms", type=int, default=1000)
    p.add_argument("--scale", type=float, default=1e6)
    p.add_argument("--seed", type=int, default=42)
    a = p.parse_args()
    dev, R = 0, a.rows
    total = a.steps + a.warmup
    d_ts = dz.DeviceArray(dev, total * R * 8)
    d_kid = dz.DeviceArray(dev, total * R * 4)
    d_v = dz.DeviceArray(dev, total * R * 8)
    dz.generate(dev, a.seed, 1_000_000, 0, total * R, a.keys, a.rows_per_ms,
                d_ts.ptr, None, d_kid.ptr, d_v.ptr)
    dz.synchronize(dev)
    is_int = a.mode.startswith("int64")
    if is_int:
        host = np.empty(R, np.float64)
        for s in range(total):
            src = at(d_v, s * R * 8)
            if _lib.lib().dz_memcpy_d2h(host.ctypes.data_as(ctypes.c_void_p),
                                        src, host.nbytes) != 0:
                raise RuntimeError("d2h failed")
            ints = np.trunc(host * a.scale).astype(np.int64)
            if _lib.lib().dz_memcpy_h2d(src,
                                        ints.ctypes.data_as(ctypes.c_void_p),
                                        ints.nbytes) != 0:
                raise RuntimeError("h2d failed")
        dz.synchronize(dev)
    names = BASE + (["stddev"] if a.mode.endswith("var") else [])
    kw = {"value_dtype": "int64"} if is_int else {}
    op = dz.WindowOp(length_ms=1000, key_kind=_lib.KEY_DENSE_INT64,
                     n_keys_hint=a.keys, device=dev,
                     aggs=[(n, 0) for n in names], **kw)

    def step(s):
        op.push_device(R, at(d_ts, s * R * 8), at(d_kid, s * R * 4),
                       at(d_v, s * R * 8), borrowed=True)
        return sum(b["n_rows"] for b in op.poll_iter())

    out_rows = 0
    for s in range(a.warmup):
        out_rows += step(s)
    op.drain()
    out_rows += sum(b["n_rows"] for b in op.poll_iter())
    dz.synchronize(dev)
    t0 = time.perf_counter()
    for s in range(a.warmup, total):
        out_rows += step(s)
    op.drain()
    out_rows += sum(b["n_rows"] for b in op.poll_iter())
    dz.synchronize(dev)
    dt = time.perf_counter() - t0
    st = op.kernel_stats()
    res = {"mode": a.mode, "aggs": names, "keys": a.keys, "rows": R,
           "steps": a.steps, "ms_per_step": round(dt / a.steps * 1e3, 3),
           "rows_per_s": round(a.steps * R / dt), "emitted_rows": out_rows,
           "regfold_launches": st["regfold"]["launches"],
           "regfold_ms_per_step": round(st["regfold"]["total_ms"] / total, 4)}
    op.finish()
    op.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
