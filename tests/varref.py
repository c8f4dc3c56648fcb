"""Pure-Python reference for the variance-family aggregates (var_samp,
var_pop, stddev_samp, stddev_pop) — TEST INFRASTRUCTURE ONLY.

Restates DataFusion's variance accumulator: a per-row Welford update of
(count, mean, m2) in row order, every operation rounded on its own. Python
floats are IEEE f64 and CPython never contracts a*b+c, so this is the
bit-exact expectation for the engine's fold. Row order, counts, window
columns and the base validity come from oracle.pyoracle.Oracle on the same
input; this module only adds the Welford columns on top of its rows.
"""
import math

import numpy as np

VAR_SAMP, VAR_POP, STDDEV_SAMP, STDDEV_POP = 5, 6, 7, 8
OPS = {"var_samp": VAR_SAMP, "var_pop": VAR_POP,
       "stddev_samp": STDDEV_SAMP, "stddev_pop": STDDEV_POP}
ALIASES = {"var_samp": "var_samp", "var_sample": "var_samp", "var": "var_samp",
           "var_pop": "var_pop", "stddev": "stddev_samp",
           "stddev_samp": "stddev_samp", "stddev_pop": "stddev_pop"}


def welford(values):
    """(count, mean, m2) after feeding `values` (valid rows, stream order)."""
    count, mean, m2 = 0, 0.0, 0.0
    for v in values:
        v = float(v)
        n = count + 1
        d1 = v - mean
        mean = d1 / float(n) + mean
        d2 = v - mean
        m2 = m2 + d1 * d2
        count = n
    return count, mean, m2


def _sqrt(x):
    # math.sqrt raises on negative input where IEEE sqrt gives NaN
    if x != x or x < 0.0:
        return math.nan
    return math.sqrt(x)


def finalize(op, count, m2):
    """(value, valid) for op code or canonical name."""
    op = OPS.get(op, op)
    if op not in (VAR_SAMP, VAR_POP, STDDEV_SAMP, STDDEV_POP):
        raise ValueError(f"not a variance op: {op!r}")
    div = count if op in (VAR_POP, STDDEV_POP) else count - 1
    if count == 0 or div == 0:
        return 0.0, 0
    # numpy scalar division: IEEE semantics for inf/nan, no ZeroDivisionError
    v = float(np.float64(m2) / np.float64(div))
    if op in (STDDEV_SAMP, STDDEV_POP):
        v = _sqrt(v)
    return v, 1


def in_own_grid(batches, ws, len_ms, slide_ms):
    """Per row of the concatenated batches: does its own batch's window list
    hold the start `ws`? A sliding grid is anchored per batch, so when the
    slide does not divide the snap unit a frame receives rows only from the
    batches whose list contains its start."""
    from tests.pyref import windows_for_range
    has = [any(s == ws for s, _e in windows_for_range(
               int(np.min(b[0])), int(np.max(b[0])), len_ms, slide_ms))
           for b in batches]
    return np.repeat(np.array(has, bool), [len(b[0]) for b in batches])


def expected(exp, batches, valids=None, slide_ms=None):
    """Welford columns for the oracle's emitted rows.

    exp: Oracle.fetch() dict for the same `batches` [(ts, key, val), ...],
    whose timestamps are non-decreasing across the whole stream, so every
    (window, key) is emitted once and a window's rows are one contiguous
    run [start <= ts < end). valids: per-batch 0/1 arrays or None.
    slide_ms: the sliding hop; needed when it does not divide the snap unit
    (in_own_grid), harmless otherwise.
    Returns {name: (values f64[n], valid u8[n])} for the four canonical
    names, row-aligned with exp."""
    ts = np.concatenate([np.asarray(b[0], np.int64) for b in batches])
    keys = np.concatenate([np.asarray(b[1], np.int64) for b in batches])
    vals = np.concatenate([np.asarray(b[2], np.float64) for b in batches])
    if valids is None:
        ok = np.ones(len(ts), bool)
    else:
        ok = np.concatenate([
            np.ones(len(b[0]), bool) if v is None else np.asarray(v, bool)
            for b, v in zip(batches, valids)])
    assert np.all(np.diff(ts) >= 0), "varref needs non-decreasing timestamps"
    n = len(exp["key"])
    out = {name: (np.zeros(n), np.zeros(n, np.uint8)) for name in OPS}
    state = {}  # (wstart, key) -> (count, m2)
    wins = sorted(set(zip(exp["window_start"].tolist(),
                          exp["window_end"].tolist())))
    for ws, we in wins:
        lo, hi = np.searchsorted(ts, [ws, we], side="left")
        own = ok[lo:hi]
        if slide_ms:
            own = own & in_own_grid(batches, ws, we - ws, slide_ms)[lo:hi]
        sel = np.flatnonzero(own) + lo
        order = sel[np.argsort(keys[sel], kind="stable")]  # row order per key
        ks = keys[order]
        cuts = np.flatnonzero(np.diff(ks)) + 1
        for seg in np.split(order, cuts):
            if len(seg):
                c, _mean, m2 = welford(vals[seg].tolist())
                state[(ws, int(keys[seg[0]]))] = (c, m2)
    seen = set()
    for r in range(n):
        g = (int(exp["window_start"][r]), int(exp["key"][r]))
        # disordered or late streams: tests/streamref.py is the reference
        assert g not in seen, "group emitted twice: late data is out of scope"
        seen.add(g)
        count, m2 = state.get(g, (0, 0.0))
        assert count == int(exp["count"][r]), (g, count, exp["count"][r])
        for name in OPS:
            v, valid = finalize(name, count, m2)
            out[name][0][r] = v
            out[name][1][r] = valid
    return out
