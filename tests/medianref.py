"""Numpy reference for the median aggregate — TEST INFRASTRUCTURE ONLY.

Restates DataFusion's median on Float64 as the engine documents it
(include/denormalized_amd.h, DZ_AGG_MEDIAN): the group's valid values sorted
by IEEE total order (-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN;
sort key = bits ^ (sign ? ~0 : 1 << 63)); n == 0 is NULL, n odd is v[n/2],
n even is (v[n/2-1] + v[n/2]) / 2.0 with one f64 add and one f64 divide.
Row set, counts, window columns and the base validity come from
oracle.pyoracle.Oracle on the same input; this module only adds the median
column on top of its rows.
"""
import numpy as np

_SIGN = np.uint64(1 << 63)


def total_order_key(values):
    """uint64 keys whose unsigned order is the IEEE total order."""
    bits = np.ascontiguousarray(values, np.float64).view(np.uint64)
    return np.where(bits >> np.uint64(63) != 0, ~bits, bits ^ _SIGN)


def median(values):
    """(value, valid) of the valid values of one group."""
    v = np.ascontiguousarray(values, np.float64)
    n = len(v)
    if n == 0:
        return 0.0, 0
    s = v[np.argsort(total_order_key(v), kind="stable")]
    if n % 2:
        return float(s[n // 2]), 1
    with np.errstate(all="ignore"):  # overflow to inf, inf + -inf = NaN
        return float((s[n // 2 - 1] + s[n // 2]) / np.float64(2.0)), 1


def expected(exp, batches, valids=None, slide_ms=None):
    """Median column for the oracle's emitted rows.

    exp: Oracle.fetch() dict for the same `batches` [(ts, key, val), ...].
    A window's rows are selected by membership, start <= ts < end, per emitted
    window, so timestamps need no order; every (window, key) must be emitted
    once (no late data reopening a closed window). valids: per-batch 0/1
    arrays or None. slide_ms: the sliding hop; needed when it does not divide
    the snap unit (varref.in_own_grid), harmless otherwise. Returns (values
    f64[n], valid u8[n]) row-aligned with exp."""
    from tests.varref import in_own_grid
    ts = np.concatenate([np.asarray(b[0], np.int64) for b in batches])
    keys = np.concatenate([np.asarray(b[1], np.int64) for b in batches])
    vals = np.concatenate([np.asarray(b[2], np.float64) for b in batches])
    if valids is None:
        ok = np.ones(len(ts), bool)
    else:
        ok = np.concatenate([
            np.ones(len(b[0]), bool) if v is None else np.asarray(v, bool)
            for b, v in zip(batches, valids)])
    n = len(exp["key"])
    out_v, out_m = np.zeros(n), np.zeros(n, np.uint8)
    state = {}  # (wstart, key) -> (median, valid, count)
    wins = sorted(set(zip(exp["window_start"].tolist(),
                          exp["window_end"].tolist())))
    for ws, we in wins:
        own = (ts >= ws) & (ts < we) & ok
        if slide_ms:
            own &= in_own_grid(batches, ws, we - ws, slide_ms)
        sel = np.flatnonzero(own)
        order = sel[np.argsort(keys[sel], kind="stable")]
        cuts = np.flatnonzero(np.diff(keys[order])) + 1
        for seg in np.split(order, cuts):
            if len(seg):
                state[(ws, int(keys[seg[0]]))] = median(vals[seg]) + (len(seg),)
    seen = set()
    for r in range(n):
        g = (int(exp["window_start"][r]), int(exp["key"][r]))
        # late data re-creating a closed window: tests/streamref.py covers it
        assert g not in seen, "group emitted twice: late data is out of scope"
        seen.add(g)
        v, m, count = state.get(g, (0.0, 0, 0))
        assert count == int(exp["count"][r]), (g, count, exp["count"][r])
        out_v[r], out_m[r] = v, m
    return out_v, out_m
