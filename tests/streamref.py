"""Row-list stream reference for every aggregate family — TEST INFRASTRUCTURE
ONLY.

A pure Python/numpy model of the windowed aggregate that keeps, per (frame,
key) group and per value column, the list of valid values in row order, and
finalises every aggregate from that list when the frame closes. Because a
group is nothing but its rows, disorder needs no special case: rows may come
in any timestamp order, and a row older than the watermark re-creates its
closed frame, which is emitted again at once holding only the late rows.

Nothing is restated that another reference already states:

  windowing             pyref.windows_for_range; the watermark (running max
                        of batch minimums), the ascending-start trigger and
                        finish follow pyref.PyRef line for line
  f64 min / max         the sequential compare loop of pyref.PyRef.push: the
                        first valid value initialises, a later one replaces
                        only on < or > (so a leading NaN sticks)
  f64 sum / avg         a left-to-right Python float loop from 0.0; sum / n
  variance family       varref.welford + varref.finalize
  median                medianref.median
  int64 columns         intref.wrap_sum, intref.fsum_rows,
                        intref.welford_step / var_finalize; signed min / max

A group exists from its first row, NULL or not; groups are emitted in
first-seen row order per frame, frames in ascending start order.
"""
import numpy as np

from tests import intref, medianref, varref
from tests.multicolref import CMP
from tests.pyref import windows_for_range

VAR_NAMES = ("var_samp", "var_pop", "stddev_samp", "stddev_pop")


def _minmax(values):
    lo = hi = values[0]
    for v in values[1:]:
        if v < lo:
            lo = v
        if v > hi:
            hi = v
    return lo, hi


def _fsum(values):
    s = 0.0
    for v in values:
        s += v
    return s


class StreamRef:
    """push(ts, keys, cols, valids): cols is one value array or a list of
    them (one per value column), valids None, one 0/1 array, or a list with
    one entry (array or None) per column. dtype "int64" takes integer value
    columns and finalises them as tests/intref.py does."""

    def __init__(self, len_ms, slide_ms=0, ncols=1, no_group=False,
                 dtype="float64"):
        assert dtype in ("float64", "int64")
        self.len_ms, self.slide_ms = len_ms, slide_ms
        self.ncols, self.no_group, self.dtype = ncols, no_group, dtype
        self.frames = {}   # start -> (end, {key: [values of col 0, ...]})
        self.watermark = None
        self.rows = []     # (key, [values of col 0, ...], wstart, wend)

    def push(self, ts, keys, cols, valids=None):
        ts = np.ascontiguousarray(ts, np.int64)
        n = len(ts)
        if n == 0:
            return
        if not isinstance(cols, (list, tuple)):
            cols = [cols]
        per_col = isinstance(valids, (list, tuple)) and all(
            v is None or hasattr(v, "__len__") for v in valids)
        if not per_col:
            assert valids is None or self.ncols == 1, "one mask per column"
            valids = [valids] * self.ncols
        assert len(cols) == len(valids) == self.ncols
        if self.dtype == "int64":
            for c in cols:
                assert np.asarray(c).dtype.kind in "iu", "integer values only"
            vals = [np.ascontiguousarray(c, np.int64).tolist() for c in cols]
        else:
            vals = [np.ascontiguousarray(c, np.float64).tolist() for c in cols]
        oks = [[True] * n if v is None else np.asarray(v).astype(bool).tolist()
               for v in valids]
        klist = ([0] * n if self.no_group
                 else np.ascontiguousarray(keys, np.int64).tolist())
        mn, mx = int(ts.min()), int(ts.max())
        for ws, we in windows_for_range(mn, mx, self.len_ms, self.slide_ms):
            if ws not in self.frames:      # whatever the watermark says
                self.frames[ws] = (we, {})
            table = self.frames[ws][1]
            for i in np.flatnonzero((ts >= ws) & (ts < we)).tolist():
                g = table.get(klist[i])
                if g is None:
                    g = table[klist[i]] = [[] for _ in range(self.ncols)]
                for c in range(self.ncols):
                    if oks[c][i]:
                        g[c].append(vals[c][i])
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

    def values(self, col=0):
        """The emitted groups' valid values of one column, row-aligned with
        fetch(): a list of lists."""
        return [r[1][col] for r in self.rows]

    def fetch(self, col=0):
        """Emitted rows as columns, for value column `col`: the names of
        pyoracle.Oracle.fetch() (key, count, min, max, avg, sum, valid,
        window_start, window_end), the four variance names each with
        '<name>_valid', and for f64 columns median (NULL where valid is 0).
        NULL cells are 0. int64 columns: min / max / sum are int64."""
        n = len(self.rows)
        ints = self.dtype == "int64"
        vt = np.int64 if ints else np.float64
        out = {
            "key": np.array([r[0] for r in self.rows], np.int64),
            "count": np.zeros(n, np.int64),
            "min": np.zeros(n, vt), "max": np.zeros(n, vt),
            "sum": np.zeros(n, vt), "avg": np.zeros(n, np.float64),
            "valid": np.zeros(n, np.uint8),
            "window_start": np.array([r[2] for r in self.rows], np.int64),
            "window_end": np.array([r[3] for r in self.rows], np.int64),
        }
        for name in VAR_NAMES:
            out[name] = np.zeros(n, np.float64)
            out[name + "_valid"] = np.zeros(n, np.uint8)
        if not ints:
            out["median"] = np.zeros(n, np.float64)
        for r, row in enumerate(self.rows):
            vs = row[1][col]
            cnt = len(vs)
            out["count"][r] = cnt
            if ints:
                m2 = 0.0
                mean = 0.0
                for i, v in enumerate(vs):
                    mean, m2 = intref.welford_step(float(v), i + 1, mean, m2)
                fin = {name: intref.var_finalize(name, cnt, m2)
                       for name in VAR_NAMES}
            else:
                c, _mean, m2 = varref.welford(vs)
                assert c == cnt
                fin = {name: varref.finalize(name, cnt, m2)
                       for name in VAR_NAMES}
            for name, (v, ok) in fin.items():
                out[name][r], out[name + "_valid"][r] = v, ok
            if cnt == 0:
                continue
            out["valid"][r] = 1
            if ints:
                out["min"][r], out["max"][r] = min(vs), max(vs)
                out["sum"][r] = intref.wrap_sum(vs)
                out["avg"][r] = intref.fsum_rows(vs) / float(cnt)
            else:
                out["min"][r], out["max"][r] = _minmax(vs)
                s = _fsum(vs)
                out["sum"][r] = s
                out["avg"][r] = s / cnt
                out["median"][r] = medianref.median(vs)[0]
        return out


def run(len_ms, slide_ms, batches, valids=None, finish=True, **kw):
    """batches: [(ts, keys, values or [values per column]), ...]; valids: per
    batch None, a 0/1 array, or a list per column. Returns the StreamRef
    after finish()."""
    first = batches[0][2]
    ncols = len(first) if isinstance(first, (list, tuple)) else 1
    r = StreamRef(len_ms, slide_ms, ncols=ncols, **kw)
    for bi, (ts, k, v) in enumerate(batches):
        r.push(ts, k, v, None if valids is None else valids[bi])
    if finish:
        r.finish()
    return r


def mask_of(cols, field):
    """The NULL mask that governs `field`: its own '<field>_valid' where it
    has one, else the row's 'valid'; count is never NULL."""
    if field == "count":
        return np.ones(len(cols["count"]), bool)
    own = field + "_valid"
    return cols[own if own in cols else "valid"].astype(bool)


def filter_rows(cols, field, cmp, literal):
    """Rows passing `field cmp literal` (multicolref.expect's filt rule): the
    value is compared as f64 and a NULL never passes. Returns (kept columns,
    keep mask)."""
    v = cols[field].astype(np.float64)
    with np.errstate(invalid="ignore"):
        keep = CMP[cmp](v, literal) & mask_of(cols, field)
    return {k: a[keep] for k, a in cols.items()}, keep


def twice(cols):
    """(window_start, key) pairs emitted more than once, in first-emission
    order, each with the row indices of its emissions."""
    seen = {}
    for r, g in enumerate(zip(cols["window_start"].tolist(),
                              cols["key"].tolist())):
        seen.setdefault(g, []).append(r)
    return {g: rows for g, rows in seen.items() if len(rows) > 1}
