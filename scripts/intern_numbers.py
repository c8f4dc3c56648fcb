"""Intern cost per launch, and step-level rows/s with the intern inside the
timed region, for the three device key kinds. One measurement per process;
prints one JSON line. scripts/intern_numbers.sh runs the set that
BASELINE.md "Intern: int64 keys" reports.

  --mode kernel  The device is idle when each push enqueues its intern (the
                 previous push is drained and the device synchronised first),
                 so the HIP-event time of the `intern` / `intern_i64` row of
                 kernel_stats() is the chain's own. The row is sampled on
                 launches 1, 9, 17, ...: launch 1 (every key new) is reported
                 as cold_ms, the mean of the later samples as steady_ms.
  --mode step    The pipelined push/poll loop of bench.py: wall time over the
                 timed steps, rows/s; intern_ms_in_pipeline is the mean of
                 the row's samples taken during the timed steps, where the
                 intern shares the device with the previous step's kernels.

Keys are k = draw % n_keys from the shared generator: "sensor_{k}" (utf8),
k itself (dense), and k * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019 mod 2^64
(i64: sparse, both signs, injective).
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

ROW_MAX = 16  # "sensor_" + at most 7 digits


def at(arr, byte_off):
    return ctypes.c_void_p(arr.ptr.value + byte_off)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=["kernel", "step"], required=True)
    p.add_argument("--kind", choices=["i64", "utf8", "dense"], required=True)
    p.add_argument("--keys", type=int, required=True)
    p.add_argument("--rows", type=int, default=8_000_000)
    p.add_argument("--steps", type=int, default=33)
    p.add_argument("--warmup", type=int, default=4)
    p.add_argument("--rows-per-ms", type=int, default=10_000)
    p.add_argument("--seed", type=int, default=42)
    a = p.parse_args()
    dev, B = 0, a.rows
    total = a.steps + (a.warmup if a.mode == "step" else 0)
    L = _lib.lib()

    d_ts = dz.DeviceArray(dev, total * B * 8)
    d_vals = dz.DeviceArray(dev, total * B * 8)
    d_keys = dz.DeviceArray(dev, total * B * 8) if a.kind == "i64" else None
    d_kid = dz.DeviceArray(dev, total * B * 4) if a.kind == "dense" else None
    dz.generate(dev, a.seed, 1_000_000, 0, total * B, a.keys, a.rows_per_ms,
                d_ts.ptr, d_keys.ptr if d_keys else None,
                d_kid.ptr if d_kid else None, d_vals.ptr)
    dz.synchronize(dev)
    if a.kind == "i64":
        for s in range(total):
            k = np.empty(B, np.uint64)
            L.dz_memcpy_d2h(k.ctypes.data_as(ctypes.c_void_p),
                            at(d_keys, s * B * 8), B * 8)
            with np.errstate(over="ignore"):
                k = k * np.uint64(0x9E3779B97F4A7C15) + \
                    np.uint64(0x632BE59BD9B4E019)
            L.dz_memcpy_h2d(at(d_keys, s * B * 8),
                            k.ctypes.data_as(ctypes.c_void_p), B * 8)
    if a.kind == "utf8":
        d_offs = dz.DeviceArray(dev, total * (B + 1) * 4)
        d_data = dz.DeviceArray(dev, total * B * ROW_MAX)
        d_lens = dz.DeviceArray(dev, B * 4)
        h_lens = np.empty(B, np.int32)
        h_offs = np.zeros(B + 1, np.int32)
        for s in range(total):
            dz.generate_utf8(dev, a.seed, s * B, B, a.keys, d_lens=d_lens.ptr)
            L.dz_memcpy_d2h(h_lens.ctypes.data_as(ctypes.c_void_p),
                            d_lens.ptr, B * 4)
            np.cumsum(h_lens, out=h_offs[1:])
            L.dz_memcpy_h2d(at(d_offs, s * (B + 1) * 4),
                            h_offs.ctypes.data_as(ctypes.c_void_p),
                            (B + 1) * 4)
            dz.generate_utf8(dev, a.seed, s * B, B, a.keys,
                             d_offsets=at(d_offs, s * (B + 1) * 4),
                             d_key_data=at(d_data, s * B * ROW_MAX))
    dz.synchronize(dev)

    kind = {"i64": _lib.KEY_INT64, "utf8": _lib.KEY_UTF8,
            "dense": _lib.KEY_DENSE_INT64}[a.kind]
    op = dz.WindowOp(length_ms=1000, key_kind=kind, n_keys_hint=a.keys,
                     device=dev)
    op.set_filter("max", ">", 113.0)

    def push(s):
        ts, v = at(d_ts, s * B * 8), at(d_vals, s * B * 8)
        if a.kind == "i64":
            op.push_device_i64(B, ts, at(d_keys, s * B * 8), v)
        elif a.kind == "utf8":
            op.push_device_utf8(B, ts, at(d_offs, s * (B + 1) * 4),
                                at(d_data, s * B * ROW_MAX), v)
        else:
            op.push_device(B, ts, at(d_kid, s * B * 4), v, borrowed=True)

    def consume():
        n = 0
        for b in op.poll_iter():
            n += b["n_rows"]
        return n

    res = {"mode": a.mode, "kind": a.kind, "keys": a.keys, "rows": B,
           "steps": a.steps}
    if a.mode == "kernel":
        row = "intern_i64" if a.kind == "i64" else "intern"
        sums = []  # summed sample ms after launches 1, 9, 17, ...
        for s in range(total):
            op.drain()
            consume()
            dz.synchronize(dev)
            push(s)
            if s % 8 == 0:
                st = op.kernel_stats()[row]
                timed = (st["launches"] + 7) // 8
                sums.append(st["total_ms"] * timed / st["launches"])
        samples = np.diff([0.0] + sums)
        res["cold_ms"] = round(float(samples[0]), 4)
        res["steady_ms"] = (round(float(samples[1:].mean()), 4)
                            if len(samples) > 1 else None)
        res["steady_samples_ms"] = [round(float(x), 4) for x in samples[1:]]
    else:
        out_rows = 0
        for s in range(a.warmup):
            push(s)
            out_rows += consume()
        op.drain()
        consume()
        dz.synchronize(dev)
        row = {"i64": "intern_i64", "utf8": "intern"}.get(a.kind)

        def sampled():  # (summed sample ms, samples) of the intern row
            st = op.kernel_stats()[row]
            timed = (st["launches"] + 7) // 8
            return st["total_ms"] * timed / st["launches"], timed
        warm = sampled() if row else None
        t0 = time.perf_counter()
        for s in range(a.warmup, total):
            push(s)
            out_rows += consume()
        op.drain()
        out_rows += consume()
        dz.synchronize(dev)
        dt = time.perf_counter() - t0
        res["rows_per_s"] = round(a.steps * B / dt)
        res["ms_per_step"] = round(dt / a.steps * 1e3, 3)
        res["emitted_rows"] = out_rows
        if row:
            # the same row inside the pipeline, samples of the timed steps
            # only: the intern shares the device with the previous step's
            # partition and fold
            end = sampled()
            res["intern_ms_in_pipeline"] = round(
                (end[0] - warm[0]) / (end[1] - warm[1]), 4)
    op.finish()
    consume()
    op.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
