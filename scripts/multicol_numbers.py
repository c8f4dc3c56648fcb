"""Step time and fold-kernel time of a window op that aggregates over several
value columns, against the single-column ops a user needed before. One
measurement per process; prints one JSON line. scripts/multicol_numbers.sh
runs the set that BASELINE.md "Several value columns" reports.

Shape: cfg2 with dense keys (8M-row steps, 10k keys, 1000 rows/ms, 1 s
tumbling window), the pipelined borrowed push/poll loop of bench.py, wall
time over the timed steps. Column 0 is the generator's reading; columns 1..3
are the same generator under other seeds.

  --mode multi --cols K   ONE op, count/min/max/avg spread over K columns:
                          K=1 all on c0; K=2 count,min on c0, max,avg on c1;
                          K=4 one aggregate per column.
  --mode split --cols K   K single-column ops (count/min/max/avg each) pushed
                          back to back over the same ts/key inputs, one per
                          column: every op re-partitions and re-emits the
                          same keys.

fold_ms_per_launch is the `regfold` row of kernel_stats() (HIP events on
every 8th launch, scaled to all launches) divided by its launches, summed
over the ops of a split run. gather_ms_per_step is the `h_trig_gather` row the
same way: push-thread wall time spent enqueueing the close gather, per step.
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

SPREAD = {1: [0, 0, 0, 0], 2: [0, 0, 1, 1], 3: [0, 1, 2, 2], 4: [0, 1, 2, 3]}
OPS = ["count", "min", "max", "avg"]


def at(arr, byte_off):
    return ctypes.c_void_p(arr.ptr.value + byte_off)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=["multi", "split"], required=True)
    p.add_argument("--cols", type=int, choices=[1, 2, 3, 4], required=True)
    p.add_argument("--keys", type=int, default=10_000)
    p.add_argument("--rows", type=int, default=8_000_000)
    p.add_argument("--steps", type=int, default=24)
    p.add_argument("--warmup", type=int, default=4)
    p.add_argument("--rows-per-ms", type=int, default=1000)
    p.add_argument("--seed", type=int, default=42)
    a = p.parse_args()
    dev, B, K = 0, a.rows, a.cols
    total = a.steps + a.warmup

    d_ts = dz.DeviceArray(dev, total * B * 8)
    d_kid = dz.DeviceArray(dev, total * B * 4)
    d_cols = [dz.DeviceArray(dev, total * B * 8) for _ in range(K)]
    dz.generate(dev, a.seed, 1_000_000, 0, total * B, a.keys, a.rows_per_ms,
                d_ts.ptr, None, d_kid.ptr, d_cols[0].ptr)
    for c in range(1, K):
        dz.generate(dev, a.seed + 1000 * c, 1_000_000, 0, total * B, a.keys,
                    a.rows_per_ms, None, None, None, d_cols[c].ptr)
    dz.synchronize(dev)

    if a.mode == "multi":
        if K == 1:
            aggs = [(o, 0) for o in OPS]
        else:
            aggs = [(o, 2 + c, o) for o, c in zip(OPS, SPREAD[K])]
        ops = [dz.WindowOp(length_ms=1000, key_kind=_lib.KEY_DENSE_INT64,
                           n_keys_hint=a.keys, device=dev, aggs=aggs)]
    else:
        ops = [dz.WindowOp(length_ms=1000, key_kind=_lib.KEY_DENSE_INT64,
                           n_keys_hint=a.keys, device=dev) for _ in range(K)]

    def push(s):
        ts, kid = at(d_ts, s * B * 8), at(d_kid, s * B * 4)
        if a.mode == "multi":
            if K > 1:
                ops[0].set_extra_values(
                    B, [at(d_cols[c], s * B * 8) for c in range(1, K)])
            ops[0].push_device(B, ts, kid, at(d_cols[0], s * B * 8),
                               borrowed=True)
        else:
            for c, op in enumerate(ops):
                op.push_device(B, ts, kid, at(d_cols[c], s * B * 8),
                               borrowed=True)

    def consume():
        n = 0
        for op in ops:
            for b in op.poll_iter():
                n += b["n_rows"]
        return n

    def stat(name):  # (summed scaled ms, launches) over the ops
        ms = ln = 0
        for op in ops:
            st = op.kernel_stats().get(name, {"total_ms": 0, "launches": 0})
            ms += st["total_ms"]
            ln += st["launches"]
        return ms, ln

    def fold():
        return stat("regfold")

    out_rows = 0
    for s in range(a.warmup):
        push(s)
        out_rows += consume()
    for op in ops:
        op.drain()
    consume()
    dz.synchronize(dev)
    f0, g0 = fold(), stat("h_trig_gather")
    t0 = time.perf_counter()
    for s in range(a.warmup, total):
        push(s)
        out_rows += consume()
    for op in ops:
        op.drain()
    out_rows += consume()
    dz.synchronize(dev)
    dt = time.perf_counter() - t0
    f1, g1 = fold(), stat("h_trig_gather")
    res = {"mode": a.mode, "cols": K, "keys": a.keys, "rows": B,
           "steps": a.steps,
           "ms_per_step": round(dt / a.steps * 1e3, 3),
           "rows_per_s": round(a.steps * B / dt),
           # per op-launch; a split step runs K of them
           "fold_ms_per_launch": round((f1[0] - f0[0]) / max(1, f1[1] - f0[1]), 4),
           "fold_launches_per_step": round((f1[1] - f0[1]) / a.steps, 2),
           "gather_ms_per_step": round((g1[0] - g0[0]) / a.steps, 4),
           "gather_launches": g1[1] - g0[1],
           "emitted_rows": out_rows}
    for op in ops:
        op.finish()
    consume()
    for op in ops:
        op.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
