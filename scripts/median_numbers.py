"""Cost of the median aggregate: an A/B on one machine, one measurement per
process, one JSON line each. BASELINE.md "Median" reports the set.

Shape: cfg2 with dense keys (8M-row steps, 10k keys, 1000 rows/ms, 1 s
tumbling window), the pipelined borrowed push/poll loop of bench.py, wall
time over the timed steps.

  --mode a       the reference example's six aggregates:
                 count, min, max, avg, median, stddev
  --mode b       the same op without median (also runs on a build that has
                 no median: it names no new symbol)
  --mode global  one global (no GROUP BY) window holding ONE group of --rows
                 rows: the single-block select over global memory. Reports
                 the wall time of finish() (the close) and the four kernels.

Kernel rows come from kernel_stats() (HIP events on every 8th launch, scaled
to all launches); h_med_wait is the host wait the append adds per batch.
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import denormalized_amd as dz  # noqa: E402
from denormalized_amd import _lib  # noqa: E402

A = ["count", "min", "max", "avg", "median", "stddev"]
B = [n for n in A if n != "median"]
MED_ROWS = ["med_count", "med_append", "med_scan", "med_place", "med_select",
            "h_med_wait"]


def at(arr, byte_off):
    return ctypes.c_void_p(arr.ptr.value + byte_off)


def med_stats(op, per):
    st = op.kernel_stats()
    return {k: {"launches": st[k]["launches"],
                "ms_per_" + per[0]: round(st[k]["total_ms"] / per[1], 4)}
            for k in MED_ROWS if k in st}


def run_global(a):
    dev, n = 0, a.rows
    d_ts = dz.DeviceArray(dev, n * 8)
    d_v = dz.DeviceArray(dev, n * 8)
    dz.generate(dev, a.seed, 1_000_000, 0, n, 1, a.rows_per_ms, d_ts.ptr,
                None, None, d_v.ptr)
    dz.synchronize(dev)
    # the stream starts at 1,000,000 ms = the start of a 1000 s window, which
    # therefore holds every row
    assert n // a.rows_per_ms < 1_000_000
    op = dz.WindowOp(length_ms=1_000_000, aggs=[("count", 0), ("median", 0)],
                     no_group=True, device=dev)
    op.push_device(n, d_ts.ptr, None, d_v.ptr, borrowed=True)
    op.drain()
    dz.synchronize(dev)
    t0 = time.perf_counter()
    op.finish()
    close_ms = (time.perf_counter() - t0) * 1e3
    outs = op.poll_all()
    res = {"mode": "global", "rows": n,
           "groups_emitted": sum(b["n_rows"] for b in outs),
           "largest_group": max(int(b["count"].max()) for b in outs),
           "close_ms": round(close_ms, 3), "kernels": med_stats(op, ("run", 1))}
    op.close()
    print(json.dumps(res), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=["a", "b", "global"], required=True)
    p.add_argument("--keys", type=int, default=10_000)
    p.add_argument("--rows", type=int, default=8_000_000)
    p.add_argument("--steps", type=int, default=24)
    p.add_argument("--warmup", type=int, default=4)
    p.add_argument("--rows-per-ms", type=int, default=1000)
    p.add_argument("--seed", type=int, default=42)
    a = p.parse_args()
    if a.mode == "global":
        return run_global(a)
    dev, R = 0, a.rows
    total = a.steps + a.warmup
    d_ts = dz.DeviceArray(dev, total * R * 8)
    d_kid = dz.DeviceArray(dev, total * R * 4)
    d_v = dz.DeviceArray(dev, total * R * 8)
    dz.generate(dev, a.seed, 1_000_000, 0, total * R, a.keys, a.rows_per_ms,
                d_ts.ptr, None, d_kid.ptr, d_v.ptr)
    dz.synchronize(dev)
    names = A if a.mode == "a" else B
    op = dz.WindowOp(length_ms=1000, key_kind=_lib.KEY_DENSE_INT64,
                     n_keys_hint=a.keys, device=dev,
                     aggs=[(n, 0) for n in names])

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
    res = {"mode": a.mode, "aggs": names, "keys": a.keys, "rows": R,
           "steps": a.steps, "ms_per_step": round(dt / a.steps * 1e3, 3),
           "rows_per_s": round(a.steps * R / dt), "emitted_rows": out_rows,
           # over all steps, warmup included
           "kernels": med_stats(op, ("step", total))}
    op.finish()
    op.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
