"""Pure Python/numpy reference for int64 value columns — TEST INFRASTRUCTURE
ONLY.

Restates, over (ts, key, int64 value, validity) streams, what the engine
documents for an op set to DZ_VALUE_INT64 (include/denormalized_amd.h,
dz_window_op_set_value_type), which in turn restates upstream DataFusion:
min/max/sum over Int64 stay Int64 (signed compare; sum is add_wrapping), avg
and the variance family cast every value to Float64 first. Per (window, key)
group, over the valid rows in row order:

  count   valid rows
  min/max signed int64 compare
  sum     np.uint64 add, which wraps, read back as int64
  avg     a Python float loop  s += float(v)  in row order, then s / float(n)
  var_*   the Welford loop with the same three operations as the kernel's
          welford_step, every one rounded on its own (CPython never contracts)

Windowing, the watermark and the emission order are tests/pyref.py's (its
windows_for_range is imported, its push/trigger discipline repeated): a group
exists as soon as it has a row, NULL or not; windows close in ascending start
order, groups in first-seen order.
"""
import math

import numpy as np

from tests.pyref import windows_for_range

U64 = np.uint64
VAR_NAMES = ("var_samp", "var_pop", "stddev_samp", "stddev_pop")


def wrap_sum(ints):
    """int64 add_wrapping of a sequence of int64 values, via np.uint64."""
    a = np.ascontiguousarray(ints, np.int64).view(U64)
    with np.errstate(over="ignore"):
        s = np.add.reduce(a, dtype=U64) if len(a) else U64(0)
    return int(np.array([s], U64).view(np.int64)[0])


def fsum_rows(ints, start=0.0):
    """f64 sum of (double)v in row order."""
    s = start
    for v in ints:
        s += float(int(v))
    return s


def avg(ints):
    """cast-then-average: fsum / (double)count, or None for no rows."""
    n = len(ints)
    return fsum_rows(ints) / float(n) if n else None


def welford_step(v, n, mean, m2):
    d1 = v - mean
    nmean = d1 / float(n) + mean
    d2 = v - nmean
    return nmean, m2 + d1 * d2


def var_finalize(name, count, m2):
    """(value, valid) under the variance family's NULL rules."""
    div = count if name.endswith("_pop") else count - 1
    if count == 0 or div == 0:
        return 0.0, 0
    v = float(np.float64(m2) / np.float64(div))
    if name.startswith("stddev"):
        v = math.nan if (v != v or v < 0.0) else math.sqrt(v)
    return v, 1


class _Group:
    __slots__ = ("cnt", "mn", "mx", "sm", "fs", "mean", "m2")

    def __init__(self):
        self.cnt, self.mn, self.mx = 0, None, None
        self.sm = U64(0)
        self.fs, self.mean, self.m2 = 0.0, 0.0, 0.0

    def merge(self, lo, hi, sm):
        """min / max / uint64 sum of the group's valid values of one batch"""
        self.mn = lo if self.mn is None or lo < self.mn else self.mn
        self.mx = hi if self.mx is None or hi > self.mx else self.mx
        with np.errstate(over="ignore"):
            self.sm = self.sm + sm

    def step(self, v):
        """one valid row, in row order: the f64 sum and the Welford state"""
        f = float(v)
        self.fs += f
        self.cnt += 1
        self.mean, self.m2 = welford_step(f, self.cnt, self.mean, self.m2)


class IntRef:
    def __init__(self, len_ms, slide_ms=0, no_group=False):
        self.len_ms, self.slide_ms, self.no_group = len_ms, slide_ms, no_group
        self.frames = {}   # start -> (end, {key: _Group}) in insertion order
        self.watermark = None
        self.rows = []     # (key, _Group, wstart, wend)

    def push(self, ts, keys, vals, valid=None):
        ts = np.ascontiguousarray(ts, np.int64)
        n = len(ts)
        if n == 0:
            return
        vals = np.asarray(vals)
        assert vals.dtype.kind in "iu", "intref takes integer values only"
        vals = np.ascontiguousarray(vals, np.int64)
        keys = (np.zeros(n, np.int64) if self.no_group
                else np.ascontiguousarray(keys, np.int64))
        ok = (np.ones(n, bool) if valid is None
              else np.asarray(valid).astype(bool))
        mn, mx = int(ts.min()), int(ts.max())
        for ws, we in windows_for_range(mn, mx, self.len_ms, self.slide_ms):
            if ws not in self.frames:
                self.frames[ws] = (we, {})
            table = self.frames[ws][1]
            sel = np.flatnonzero((ts >= ws) & (ts < we))
            if not len(sel):
                continue
            order = sel[np.argsort(keys[sel], kind="stable")]
            starts = np.r_[0, np.flatnonzero(np.diff(keys[order])) + 1]
            # groups enter the table in first-seen row order, NULL rows too
            for j in np.argsort(order[starts], kind="stable").tolist():
                k = int(keys[order[starts[j]]])
                if k not in table:
                    table[k] = _Group()
            vo = order[ok[order]]      # valid rows, by key, row order inside
            if not len(vo):
                continue
            vk, vv = keys[vo], vals[vo]
            vs = np.r_[0, np.flatnonzero(np.diff(vk)) + 1]
            lo = np.minimum.reduceat(vv, vs)
            hi = np.maximum.reduceat(vv, vs)
            with np.errstate(over="ignore"):
                sm = np.add.reduceat(vv.view(U64), vs, dtype=U64)
            for k, a, b, c in zip(vk[vs].tolist(), lo.tolist(), hi.tolist(),
                                  sm):
                table[k].merge(a, b, c)
            for k, v in zip(vk.tolist(), vv.tolist()):
                table[k].step(v)
        if self.watermark is None or self.watermark <= mn:
            self.watermark = mn
        self._trigger()

    def _trigger(self):
        if self.watermark is None:
            return
        for ws in sorted(self.frames):
            we, table = self.frames[ws]
            if self.watermark >= we:
                for k, g in table.items():
                    self.rows.append((k, g, ws, we))
                del self.frames[ws]

    def finish(self):
        mx = self.watermark or 0
        for _ws, (we, _t) in self.frames.items():
            mx = max(mx, we)
        self.watermark = mx
        self._trigger()

    def fetch(self):
        """Emitted rows as columns: key, count, min/max/sum (int64, 0 where
        NULL), avg (f64), valid, the four variance names with '<name>_valid',
        window_start, window_end."""
        n = len(self.rows)
        out = {
            "key": np.array([r[0] for r in self.rows], np.int64),
            "count": np.array([r[1].cnt for r in self.rows], np.int64),
            "min": np.array([r[1].mn or 0 for r in self.rows], np.int64),
            "max": np.array([r[1].mx or 0 for r in self.rows], np.int64),
            "sum": np.array([r[1].sm for r in self.rows], U64).view(np.int64)
            if n else np.zeros(0, np.int64),
            "avg": np.array([r[1].fs / float(r[1].cnt) if r[1].cnt else 0.0
                             for r in self.rows], np.float64),
            "valid": np.array([1 if r[1].cnt else 0 for r in self.rows],
                              np.uint8),
            "window_start": np.array([r[2] for r in self.rows], np.int64),
            "window_end": np.array([r[3] for r in self.rows], np.int64),
        }
        for name in VAR_NAMES:
            fin = [var_finalize(name, r[1].cnt, r[1].m2) for r in self.rows]
            out[name] = np.array([f[0] for f in fin], np.float64)
            out[name + "_valid"] = np.array([f[1] for f in fin], np.uint8)
        return out


def run(len_ms, slide_ms, batches, valids=None, no_group=False):
    """batches: [(ts, keys, int values), ...]; valids: per-batch 0/1 arrays
    or None. Returns IntRef.fetch() after finish()."""
    r = IntRef(len_ms, slide_ms, no_group)
    for bi, (ts, k, v) in enumerate(batches):
        r.push(ts, k, v, None if valids is None else valids[bi])
    r.finish()
    return r.fetch()
